// dpg_chol.hip -- supernodal multifrontal Cholesky of the pose-graph normal equations on gfx950.
//
// This file: the kernels (factorization, solves, selected inverse, joint marginals) and the host
// driver (CholDev, the upload, one launch helper per kernel, the solve / selected-inverse /
// marginals / joint-marginals entry points).
// The host planner that builds every index table the kernels follow is dpg_chol_plan.cpp (plain
// C++); the records, constants and cost model both sides share are in dpg_chol_plan.h.
//
// The CHOLESKY solve that GTSAM runs inside GaussNewtonOptimizer / ISAM2 as a
// level-scheduled GPU factorization: the symbolic analysis (dpg_chol_sym.cpp) and the per-level
// task lists run once per sparsity pattern; each GN iteration then runs, per elimination-tree
// level, task-list kernels over all fronts of the level (dense fronts are column-major in HBM):
//   assemble: one workgroup per (front, 32-column tile), built in LDS: zero, scatter the
//             original 3x3 blocks of H, add the children's update matrices child by child
//             (deterministic order, no atomics), store once;
//   then per 48-column panel step:
//     panel:  one workgroup per front, one panel row per thread in registers, right-looking
//             by 3x3 block columns;
//     update: one workgroup per 32x32 tile of every front's trailing lower triangle (SYRK),
//             so a large front's Schur complement is spread over many CUs;
//   forward:  L y = -g, ONE launch: fronts as a DAG (children's pending row updates gathered,
//             diagonal blocks solved by one wave from LDS, L21 y handed to the parent);
//   backward: L^T x = y, ONE launch, top-down (ancestors' x gathered by row position).
// fp64 throughout, explicit fma in the inner products (this file is held to a tolerance, not to
// bit-exactness; the build keeps -ffp-contract=off for the ICP kernels); the fronts of one
// factorization stay resident in HBM (tens of MB).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dpg_chol_plan.h"
#include "dpg_ctx.h"

using namespace dpg_chol;   // the plan's records and the tile / panel constants (dpg_chol_plan.h)

namespace {

// Phase timestamps (timing builds of tools/chol_bench only): workgroup 0 of launch `pid` writes
// wall_clock64() (100 MHz) into slot [pid][k].
#ifdef DPG_CHOL_TIMING
constexpr int kProfSlots = 40;
__device__ unsigned long long g_prof[4096 * kProfSlots];
constexpr int kProfL = 512, kProfW = 2048;
__device__ unsigned long long g_span[kProfL * kProfW * 2];   // per launch, per workgroup: start, end
#define PROF_MARK(pid, k)                                                                       \
    do {                                                                                        \
        if (blockIdx.x == 0 && threadIdx.x == 0 && (pid) < 4096) g_prof[(pid) * kProfSlots + (k)] = wall_clock64(); \
    } while (0)
#define PROF_BEGIN(pid) do { if (threadIdx.x == 0 && (pid) < kProfL && blockIdx.x < kProfW) g_span[((size_t)(pid) * kProfW + blockIdx.x) * 2] = wall_clock64(); } while (0)
#define PROF_END(pid) do { if (threadIdx.x == 0 && (pid) < kProfL && blockIdx.x < kProfW) g_span[((size_t)(pid) * kProfW + blockIdx.x) * 2 + 1] = wall_clock64(); } while (0)
// per-front phase stamps of the fused kernel: [front][0 claim, 1 children ready, 2 assembled,
// 3 factored, 4 done]
__device__ unsigned long long g_front[16384 * 8];
#define FT_MARK(s, k) do { if (threadIdx.x == 0 && (s) < 16384) g_front[(s) * 8 + (k)] = wall_clock64(); } while (0)
// per-panel stamps of large fronts: [front][panel][0 wake, 1 loaded, 2 tile updated, 3 factored, 4 published]
__device__ unsigned long long g_panel[16384 * 16 * 8];
__device__ unsigned long long g_steps[16384 * 16 * 8];
#define ST_MARK(s, p, k) do { if (threadIdx.x == 0 && (s) < 16384 && (p) < 16 && (k) < 8) g_steps[((s) * 16 + (p)) * 8 + (k)] = wall_clock64(); } while (0)
#define PN_MARK(s, p, k) do { if (threadIdx.x == 0 && (s) < 16384 && (p) < 16) g_panel[((s) * 16 + (p)) * 8 + (k)] = wall_clock64(); } while (0)
// per-front stamps of the backward solve: [front][0 claim, 1 parent ready, 2 z updated, 3 solved, 4 done]
__device__ unsigned long long g_bwd[16384 * 8];
#define BW_MARK(s, k) do { if (threadIdx.x == 0 && (s) < 16384) g_bwd[(s) * 8 + (k)] = wall_clock64(); } while (0)
#else
#define BW_MARK(s, k) do { } while (0)
#define FT_MARK(s, k) do { } while (0)
#define PN_MARK(s, p, k) do { } while (0)
#define ST_MARK(s, p, k) do { } while (0)
#define PROF_MARK(pid, k) do { } while (0)
#define PROF_BEGIN(pid) do { } while (0)
#define PROF_END(pid) do { } while (0)
#endif

// ---- numeric factorization: three task-list kernels per elimination-tree level ----
// (task lists are built once per sparsity pattern by the planner, dpg_chol_plan.cpp)

// assembly: one workgroup per (front, kCT-column tile), built in LDS: zeroed, the original H
// blocks scattered in, then each child's update-matrix entries that land in the tile's columns
// (contiguous child columns [ja, jb), precomputed) added child by child -- within a child the
// map is injective, so all its entries are in flight at once; an LDS barrier between children
// fixes the summation order.  The finished tile is stored once, coalesced.
__global__ __launch_bounds__(kT) void chol_assemble(const AsmTask* __restrict__ tasks,
                                                    const AsmChild* __restrict__ tchild,
                                                    const SnDev* __restrict__ sns,
                                                    const OEnt* __restrict__ omap, const double* __restrict__ hb,
                                                    const int32_t* __restrict__ relmap, double* __restrict__ fronts,
                                                    int pid) {
    extern __shared__ __attribute__((aligned(16))) double T[];   // [kCT][m3], column-major
    const int tid = threadIdx.x;
    PROF_BEGIN(pid);
    PROF_MARK(pid, 0);
    const AsmTask tk = tasks[blockIdx.x];
    const SnDev S = sns[tk.s];
    const int m3 = 3 * (S.k + S.r);
    const int c0 = tk.c0, nc = min(c0 + kCT, m3) - c0;
    for (int e = tid; e < nc * m3; e += kT) T[e] = 0.0;
    __syncthreads();
    PROF_MARK(pid, 1);
    for (int q = tid; q < (tk.om_e - tk.om_b) * 9; q += kT) {
        const OEnt o = omap[tk.om_b + q / 9];
        const int ii = (q % 9) / 3, jj = q % 3;
        const int row = 3 * o.a + ii, col = 3 * o.b + jj;
        if (col < c0 || col >= c0 + nc || row < col) continue;
        const double* B = hb + 9 * (int64_t)o.u;
        T[(col - c0) * m3 + row] = o.tr ? B[3 * jj + ii] : B[3 * ii + jj];
    }
    PROF_MARK(pid, 2);
    for (int q = 0; q < tk.ch_cnt; ++q) {
        __syncthreads();
        const AsmChild ch = tchild[tk.ch_off + q];
        const SnDev C = sns[ch.c];
        const int r3c = 3 * C.r, k3c = 3 * C.k, m3c = 3 * (C.k + C.r);
        const int32_t* rm = relmap + C.rows_off;
        const double* Fc = fronts + C.front_off + (int64_t)k3c * m3c + k3c;
        const int nj = ch.jb - ch.ja;
        for (int e = tid; e < nj * r3c; e += kT) {
            const int jl = e / r3c, i = e - jl * r3c, j = ch.ja + jl;
            if (i < j) continue;
            const int pj = 3 * rm[j / 3] + j % 3, pi = 3 * rm[i / 3] + i % 3;
            T[(pj - c0) * m3 + pi] += Fc[(int64_t)j * m3c + i];
        }
    }
    __syncthreads();
    PROF_MARK(pid, 3);
    double* F = fronts + S.front_off + (int64_t)c0 * m3;
    for (int e = tid; e < nc * m3; e += kT) {
        const int jl = e / m3, row = e - jl * m3;
        if (row >= c0 + jl) F[e] = T[e];
    }
    PROF_MARK(pid, 4);
    __syncthreads();
    PROF_END(pid);
}

// 1/sqrt(d) from the hardware estimate (relative error ~5e-8) and ONE third-order correction:
// with e = 1 - d y^2, 1/sqrt(d) = y (1 - e)^(-1/2) = y (1 + e/2 + 3e^2/8 + O(e^3)), the O(e^3) term
// ~1e-22 -- full fp64 precision in 4 dependent operations (two Newton steps take 6).
__device__ __forceinline__ double rsqrt_nr(double d) {
    const double y = __builtin_amdgcn_rsq(d);
    const double e = fma(-(d * y), y, 1.0);
    return fma(y * e, fma(e, 0.375, 0.5), y);
}

// Cholesky factor of a 3x3 SPD block and the inverse of that factor, from the block's leading
// minors (d00, M2, det): the three reciprocal square roots are independent, so the dependent chain
// is about a third of the column-by-column one (a wave64 fp64 op is ~32 cycles of latency).
// Branch-free: a non-positive minor only raises `bad` (the solve then reports failure).
struct Chol3 { double l00, l10, l11, l20, l21, l22, m00, m10, m11, m20, m21, m22; };
__device__ __forceinline__ Chol3 chol3(double d00, double d10, double d11, double d20, double d21, double d22,
                                       bool& bad) {
    const double M2 = fma(d00, d11, -d10 * d10);
    const double c0 = fma(d11, d22, -d21 * d21), c1 = fma(d10, d22, -d21 * d20), c2 = fma(d10, d21, -d11 * d20);
    const double det = fma(d00, c0, fma(-d10, c1, d20 * c2));
    bad |= !(d00 > 0.0 && M2 > 0.0 && det > 0.0);
    const double r0 = rsqrt_nr(d00), r1 = rsqrt_nr(M2), r2 = rsqrt_nr(det);
    Chol3 L;
    L.l00 = d00 * r0;                  // sqrt(d00)
    const double s2 = M2 * r1;         // sqrt(M2)
    L.l11 = s2 * r0;                   // sqrt(M2 / d00)
    L.l22 = (det * r2) * r1;           // sqrt(det / M2)
    L.m00 = r0;
    L.m11 = L.l00 * r1;                // sqrt(d00 / M2)
    L.m22 = s2 * r2;                   // sqrt(M2 / det)
    L.l10 = d10 * r0;
    L.l20 = d20 * r0;
    L.l21 = fma(-L.l20, L.l10, d21) * L.m11;
    L.m10 = -L.l10 * (L.m00 * L.m11);
    L.m21 = -L.l21 * (L.m11 * L.m22);
    L.m20 = fma(L.l10, L.l21, -L.l20 * L.l11) * (L.m00 * L.m11 * L.m22);
    return L;
}

// panel: one workgroup per front, one panel row per thread in registers (NT >= rows), right-
// looking by 3x3 BLOCK columns (the system is 3x3-blocked, so panels are too): every thread
// factors the 3x3 diagonal block itself, solves its own row's three entries, and the panel's block
// rows are broadcast through LDS -- two barriers per three columns.  The block loop stays rolled
// (compact code: these launches run on cold instruction caches): each step shifts the register
// row by three so the current block is always p[0..2], and finished entries go straight to HBM.
// The trailing matrix is left to chol_update.
template <int NT>
__global__ __launch_bounds__(NT) void chol_panel(const Task2* __restrict__ tasks, const SnDev* __restrict__ sns,
                                                 double* __restrict__ fronts, int32_t* __restrict__ status, int pid) {
    __shared__ double s_d[6];          // the current diagonal block (lower: 00 10 11 20 21 22)
    __shared__ double4 s_l[kNB];       // L(c, 3b .. 3b+2) of the panel's own rows (w unused)
    const int i = threadIdx.x;
    const Task2 tk = tasks[blockIdx.x];
    const SnDev S = sns[tk.x];
    const int m3 = 3 * (S.k + S.r), k3 = 3 * S.k;
    const int j0 = tk.y, w = min(kNB, k3 - j0), R = m3 - j0;
    double* F = fronts + S.front_off + (int64_t)j0 * m3 + j0;
    PROF_BEGIN(pid);
    PROF_MARK(pid, 0);
    double p[kNB];
#pragma unroll
    for (int c = 0; c < kNB; ++c) p[c] = (i < R && c < w && c <= i) ? F[(int64_t)c * m3 + i] : 0.0;
    PROF_MARK(pid, 1);
    bool bad = false;
#pragma unroll 1
    for (int c0 = 0; c0 < w; c0 += 3) {
        PROF_MARK(pid, 2 + c0 / 3);
        if (i == c0) s_d[0] = p[0];
        if (i == c0 + 1) { s_d[1] = p[0]; s_d[2] = p[1]; }
        if (i == c0 + 2) { s_d[3] = p[0]; s_d[4] = p[1]; s_d[5] = p[2]; }
        __syncthreads();
        if (c0 == 3) PROF_MARK(pid, 22);
        double d00 = s_d[0], d10 = s_d[1], d11 = s_d[2], d20 = s_d[3], d21 = s_d[4], d22 = s_d[5];
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
        double x0 = 0.0, x1 = 0.0, x2 = 0.0;
        if (i == c0) { x0 = l00; }
        else if (i == c0 + 1) { x0 = l10; x1 = l11; }
        else if (i == c0 + 2) { x0 = l20; x1 = l21; x2 = l22; }
        else if (i > c0 + 2 && i < R) {
            x0 = p[0] * i00;
            x1 = (p[1] - x0 * l10) * i11;
            x2 = (p[2] - x0 * l20 - x1 * l21) * i22;
        }
        if (i >= c0 && i < R) {
            F[(int64_t)c0 * m3 + i] = x0;
            if (i >= c0 + 1) F[(int64_t)(c0 + 1) * m3 + i] = x1;
            if (i >= c0 + 2) F[(int64_t)(c0 + 2) * m3 + i] = x2;
        }
        if (c0 == 3) PROF_MARK(pid, 23);
        if (i > c0 + 2 && i < w) s_l[i] = make_double4(x0, x1, x2, 0.0);
        __syncthreads();
        if (c0 == 3) PROF_MARK(pid, 24);
        const bool upd = i > c0 + 2 && i < R;
#pragma unroll
        for (int c = 3; c < kNB; ++c) {
            const int cc = c0 + c;
            double v = p[c];
            if (upd && cc < w && cc <= i) {
                const double4 l = s_l[cc];
                v = fma(-x0, l.x, v);
                v = fma(-x1, l.y, v);
                v = fma(-x2, l.z, v);
            }
            p[c - 3] = v;
        }
        p[kNB - 3] = p[kNB - 2] = p[kNB - 1] = 0.0;
        if (c0 == 3) PROF_MARK(pid, 25);
    }
    if (bad && i == 0) atomicExch(status, 1);
    PROF_MARK(pid, 20);
    __syncthreads();
    PROF_END(pid);
}

// update: one workgroup per 32x32 tile (rows i0.., cols l0..) of a front's trailing lower
// triangle: F(i, l) -= sum_c L(i, j0 + c) L(l, j0 + c) over the panel's w columns.
__global__ __launch_bounds__(kT) void chol_update(const Task4* __restrict__ tasks, const SnDev* __restrict__ sns,
                                                  double* __restrict__ fronts, int pid) {
    PROF_BEGIN(pid);
    PROF_MARK(pid, 0);
    __shared__ double A[kNB][33], B[kNB][33];
    const int tid = threadIdx.x;
    const Task4 tk = tasks[blockIdx.x];
    const SnDev S = sns[tk.x];
    const int m3 = 3 * (S.k + S.r), k3 = 3 * S.k;
    const int j0 = tk.y, w = min(kNB, k3 - j0), i0 = tk.z, l0 = tk.w;
    double* F = fronts + S.front_off;
    for (int e = tid; e < kNB * 32; e += kT) {
        const int c = e >> 5, rr = e & 31;
        A[c][rr] = (c < w && i0 + rr < m3) ? F[(int64_t)(j0 + c) * m3 + i0 + rr] : 0.0;
        B[c][rr] = (c < w && l0 + rr < m3) ? F[(int64_t)(j0 + c) * m3 + l0 + rr] : 0.0;
    }
    __syncthreads();
    const int tx = tid & 31, ty = tid >> 5;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < w; ++c) {
        const double a = A[c][tx];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = fma(a, B[c][4 * ty + q], acc[q]);
    }
    const int i = i0 + tx;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int l = l0 + 4 * ty + q;
        if (i < m3 && l < m3 && i >= l) F[(int64_t)l * m3 + i] -= acc[q];
    }
#ifdef DPG_CHOL_TIMING
    __syncthreads();
    PROF_END(pid);
#endif
}

// ---- triangular solves: ONE launch each, fronts as a dependency DAG ----
// Workgroups claim fronts through an atomic ticket in topological order (forward: leaves first;
// backward: root first), so a workgroup only ever waits on fronts already claimed by running
// workgroups.  Hand-off (cdna_hip_programming.md Guideline 16): the payload is written with
// agent-scope (sc1, write-through) stores, drained (s_waitcnt vmcnt(0)) and the workgroup
// synchronised before ONE lane signals with an agent-scope atomic; the consumer polls relaxed,
// then one agent-scope acquire, then agent-scope loads.  Every spin is bounded: on timeout the
// status word gets 2 and the solve reports failure instead of hanging.
using u64 = unsigned long long;

__device__ __forceinline__ void st_agent(double* p, double v) {
    __hip_atomic_store(reinterpret_cast<u64*>(p), (u64)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_agent(double* p) {
    return __longlong_as_double(
        (long long)__hip_atomic_load(reinterpret_cast<u64*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
// 16-B write-through (sc1) accesses of a front: a buffer descriptor over the whole front (front
// offsets are even, so its base is 16-B aligned) and element pairs (e, e + 1), e even.  An 8-B sc1
// access moves 0.54-0.70x the bytes of a 16-B one per instruction, an 8-B sc1 store ~1/2.7
// (MI355X_MICROARCH.md, inter-workgroup visibility).  A column segment of a front is covered by the
// aligned pairs that overlap it; the element a pair holds outside the segment is the row above it
// in the same column or row 0 of the next column (both above the diagonal: never read as data) or
// the front's padding.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t front_rsrc(const double* F, int m3) {
    const uint64_t p = reinterpret_cast<uint64_t>(F);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)p);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(p >> 32));
    const int bytes = __builtin_amdgcn_readfirstlane(((m3 * m3 + 1) & ~1) * 8);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, bytes, 0x00020000);
}
__device__ __forceinline__ double2 ld2_sc1(__amdgpu_buffer_rsrc_t r, uint32_t e) {
    return __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(r, e * 8u, 0, 16));
}
__device__ __forceinline__ void st2_sc1(__amdgpu_buffer_rsrc_t r, uint32_t e, double x, double y) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, make_double2(x, y)), r, e * 8u, 0, 16);
}

// Poll without the agent acquire: every handed-off byte the waiting workgroup reads is stored sc1
// by its producer and loaded sc1 (ld_agent) here, so the L1 is never consulted for it (Guideline
// 16, the sc1-load form); the wavefront fence only keeps the compiler from hoisting those loads.
__device__ __forceinline__ void wait_geq_sc1(int32_t* w, int32_t target, int32_t* status) {
    unsigned spins = 0;
    while (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1u << 25)) {
            atomicExch(status, 2);
            break;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// A pipelined Gauss-Newton loop (dpg_gn_pipe.h) enqueues both solve paths of an iteration before
// the previous one is read: gate[0] = the iteration runs, gate[1] = it reuses the factor.  mode 0
// runs when active, 1 when active and refactoring, 2 when active and reusing; no gate: always.
__device__ __forceinline__ bool gate_off(const int32_t* gate, int mode) {
    if (!gate) return false;
    const int32_t a = gate[0], r = gate[1];   // written by an earlier launch
    return !a || (mode == 1 && r) || (mode == 2 && !r);
}

__device__ __forceinline__ int claim_lds(const int32_t* order, int32_t* ticket, int* slot) {
    if (threadIdx.x == 0) *slot = order[atomicAdd(ticket, 1)];
    __syncthreads();
    return *slot;
}

// 16-lane groups: sum of a partial over the group (xor butterfly: every lane gets the total)
__device__ __forceinline__ double group16_sum(double a) {
    a += __shfl_xor(a, 8, 16);
    a += __shfl_xor(a, 4, 16);
    a += __shfl_xor(a, 2, 16);
    a += __shfl_xor(a, 1, 16);
    return a;
}

// ---- L11^-1 of the large fronts (opts.solve_inv_cols) ----
// The triangular solves spend their critical path in the top fronts' diagonal parts: a chain of
// dependent substitution steps per 64-column block, each waiting on its block's loads (profiles/r05
// chol timing: 59 of the backward's 122 us).  After each factorization this kernel inverts L11 of
// every front with at least solve_inv_cols pivot columns; the solves then apply it as ONE product
// (all loads in flight at once).  Task (s, j0): columns [j0, j0 + kInvCols) of X = L11^-1 by
// column-parallel forward substitution, ascending i (a fixed summation order).
// One WAVE per column j of X = L11^-1 (four per workgroup): lane l owns rows j + l + 64 q (q < 3:
// fronts up to 192 pivot columns); step i broadcasts x_i from its owner (one readlane) and every lane
// adds L(r, i) x_i to its rows r > i.  L's columns come straight from the fronts (L2), 16 steps'
// worth loaded ahead into registers; no LDS, so many columns run per compute unit.
constexpr int kInvThreads = 64 * kInvCols;
constexpr int kInvAhead = 16;            // steps of L loaded ahead
__device__ __forceinline__ double rdlane_(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
__global__ __launch_bounds__(kInvThreads) void chol_inv_l11(const Task2* __restrict__ tasks, const SnDev* __restrict__ sns,
                                                            const double* __restrict__ fronts, double* __restrict__ linv,
                                                            const int32_t* gate) {
    if (gate_off(gate, 1)) return;
    const Task2 tk = tasks[blockIdx.x];
    const SnDev S = sns[tk.x];
    const int lane = threadIdx.x & 63;
    const int j = tk.y + (int)(threadIdx.x >> 6);      // this wave's column
    const int m3 = 3 * (S.k + S.r), k3 = 3 * S.k;
    if (j >= k3) return;                                // whole wave
    const int nr = k3 - j;                              // rows j .. k3 - 1
    const double* F = fronts + S.front_off;
    double* Li = linv + S.inv;
    double sacc[kInvMaxQ], xo[kInvMaxQ], rd[kInvMaxQ];
#pragma unroll
    for (int q = 0; q < kInvMaxQ; ++q) {
        const int b = lane + 64 * q;
        sacc[q] = xo[q] = 0.0;
        rd[q] = b < nr ? 1.0 / F[(int64_t)(j + b) * m3 + j + b] : 0.0;
    }
    // L(j + b, j + a) of this lane's rows b = lane + 64 q, 0 where b <= a or past the front
    auto ld = [&](int a, int q) -> double {
        const int b = lane + 64 * q;
        const bool in = b > a && b < nr && a < nr;
        const double t = F[(int64_t)(j + (a < nr ? a : 0)) * m3 + j + (in ? b : 0)];
        return in ? t : 0.0;
    };
    double cur[kInvAhead][kInvMaxQ], nxt[kInvAhead][kInvMaxQ];
#pragma unroll
    for (int u = 0; u < kInvAhead; ++u)
#pragma unroll
        for (int q = 0; q < kInvMaxQ; ++q) cur[u][q] = ld(u, q);
    for (int a0 = 0; a0 < nr; a0 += kInvAhead) {
#pragma unroll
        for (int u = 0; u < kInvAhead; ++u)   // the next 16 steps' columns, in flight during these 16
#pragma unroll
            for (int q = 0; q < kInvMaxQ; ++q) nxt[u][q] = ld(a0 + kInvAhead + u, q);
#pragma unroll
        for (int u = 0; u < kInvAhead; ++u) {
            const int a = a0 + u;                       // step: row j + a
            if (a >= nr) break;                         // (uniform)
            const int own = a & 63, qa = a >> 6;
            double s_own = sacc[0], r_own = rd[0];
#pragma unroll
            for (int q = 1; q < kInvMaxQ; ++q)
                if (qa == q) { s_own = sacc[q]; r_own = rd[q]; }
            const double v = a == 0 ? r_own : -s_own * r_own;   // meaningful on lane own
#pragma unroll
            for (int q = 0; q < kInvMaxQ; ++q)
                if (qa == q && lane == own) xo[q] = v;
            const double x = rdlane_(v, own);
#pragma unroll
            for (int q = 0; q < kInvMaxQ; ++q) sacc[q] = fma(cur[u][q], x, sacc[q]);   // (0 above the rows)
        }
#pragma unroll
        for (int u = 0; u < kInvAhead; ++u)
#pragma unroll
            for (int q = 0; q < kInvMaxQ; ++q) cur[u][q] = nxt[u][q];
    }
#pragma unroll
    for (int q = 0; q < kInvMaxQ; ++q) {
        const int b = lane + 64 * q;
        if (b < nr) Li[(int64_t)j * k3 + j + b] = xo[q];
    }
}

// y[0, k3) <- L11^-1 y (tmp: k3 doubles of LDS): one thread per output row, the columns in
// ascending order over four accumulators; the loads of a column are contiguous across the rows
__device__ __forceinline__ void inv_apply_lower(const double* __restrict__ Li, int k3, double* y, double* tmp) {
    const int tid = threadIdx.x;
    for (int t = tid; t < k3; t += kT) tmp[t] = y[t];
    __syncthreads();
    for (int i = tid; i < k3; i += kT) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int k = 0;
#pragma unroll 2
        for (; k + 3 <= i; k += 4) {
            a0 = fma(Li[(int64_t)k * k3 + i], tmp[k], a0);
            a1 = fma(Li[(int64_t)(k + 1) * k3 + i], tmp[k + 1], a1);
            a2 = fma(Li[(int64_t)(k + 2) * k3 + i], tmp[k + 2], a2);
            a3 = fma(Li[(int64_t)(k + 3) * k3 + i], tmp[k + 3], a3);
        }
        for (; k <= i; ++k) a0 = fma(Li[(int64_t)k * k3 + i], tmp[k], a0);
        y[i] = (a0 + a1) + (a2 + a3);
    }
    __syncthreads();
}
// z[0, k3) <- L11^-T z (tmp: k3 doubles of LDS): 16 lanes per output k, the dot down column k of
// L11^-1 (rows k .. k3, contiguous)
__device__ __forceinline__ void inv_apply_upper(const double* __restrict__ Li, int k3, double* z, double* tmp) {
    const int tid = threadIdx.x, g = tid >> 4, gl = tid & 15;
    for (int t = tid; t < k3; t += kT) tmp[t] = z[t];
    __syncthreads();
    for (int k0 = 0; k0 < k3; k0 += kT / 16) {
        const int k = k0 + g;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        if (k < k3) {
            const double* cl = Li + (int64_t)k * k3;
            int i = k + gl;
#pragma unroll 2
            for (; i + 48 < k3; i += 64) {
                a0 = fma(cl[i], tmp[i], a0);
                a1 = fma(cl[i + 16], tmp[i + 16], a1);
                a2 = fma(cl[i + 32], tmp[i + 32], a2);
                a3 = fma(cl[i + 48], tmp[i + 48], a3);
            }
            for (; i < k3; i += 16) a0 = fma(cl[i], tmp[i], a0);
        }
        const double a = group16_sum((a0 + a1) + (a2 + a3));
        if (k < k3 && gl == 0) z[k] = a;
    }
    __syncthreads();
}

// forward: L y = -g.  A front gathers its children's pending row updates (child order: fixed
// summation order), solves its diagonal blocks (one wave, LDS), then hands L21 y to its parent.
__device__ __forceinline__ double rdlane(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// The diagonal block at (jb, jb) of a front (bw x bw) into LDS (leading dimension kSB), padded
// to nb = chain_len(bw): its STRICT lower triangle (zero elsewhere and past bw), and the
// reciprocals of its diagonal (0 past bw).
__device__ __forceinline__ int chain_len(int bw) { return bw <= 8 ? 8 : bw <= 16 ? 16 : bw <= 32 ? 32 : 64; }
__device__ __forceinline__ void load_diag(double* D, double* rd, const double* F, int m3, int jb, int bw) {
    const int nb = chain_len(bw);
    constexpr int kPer = kSB * kSB / kT;   // every load of the block in flight at once (8 per thread)
    double v[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int e = threadIdx.x + kT * q, i = e % nb, j = e / nb;
        v[q] = (e < nb * nb && i < bw && j < bw && i >= j) ? F[(int64_t)(jb + j) * m3 + jb + i] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int e = threadIdx.x + kT * q, i = e % nb, j = e / nb;
        if (e < nb * nb) {
            D[j * kSB + i] = i > j ? v[q] : 0.0;
            if (i == j) rd[j] = j < bw ? 1.0 / v[q] : 0.0;
        }
    }
}

// One wave solves the padded unit-scaled triangle by a readlane -> fma chain; lane = row, the
// lane's scaled entries in registers (lanes >= N compute garbage nobody reads).
// forward (L y = b):  yl_i -= L(i, j) / L(j, j) * yl_j, j ascending; y = yl / L_ii afterwards
// rl: this lane's reciprocal of the block's diagonal (0 past bw), broadcast per column by readlane
// (scalar operands: the 64-step chains fit two waves per SIMD)
template <int N>
__device__ __forceinline__ double fwd_chain(const double* D, double rl, double yl, int lane) {
    double dr[N];
#pragma unroll
    for (int j = 0; j < N; ++j) dr[j] = D[j * kSB + lane] * rdlane(rl, j);
#pragma unroll
    for (int j = 0; j < N; ++j) yl = fma(-dr[j], rdlane(yl, j), yl);
    return yl;
}
// backward (L^T x = z): zl_i -= L(j, i) / L(j, j) * zl_j, j descending; x = zl / L_ii afterwards
template <int N>
__device__ __forceinline__ double bwd_chain(const double* D, double rl, double zl, int lane) {
    double dr[N];
#pragma unroll
    for (int j = 0; j < N; ++j) dr[j] = D[lane * kSB + j] * rdlane(rl, j);
#pragma unroll
    for (int j = N - 1; j >= 0; --j) zl = fma(-dr[j], rdlane(zl, j), zl);
    return zl;
}
template <bool kFwd>
__device__ __forceinline__ double run_chain(const double* D, double rl, double v, int lane, int bw) {
    const int nb = chain_len(bw);
    if constexpr (kFwd)
        return nb == 8 ? fwd_chain<8>(D, rl, v, lane) : nb == 16 ? fwd_chain<16>(D, rl, v, lane)
             : nb == 32 ? fwd_chain<32>(D, rl, v, lane) : fwd_chain<64>(D, rl, v, lane);
    else
        return nb == 8 ? bwd_chain<8>(D, rl, v, lane) : nb == 16 ? bwd_chain<16>(D, rl, v, lane)
             : nb == 32 ? bwd_chain<32>(D, rl, v, lane) : bwd_chain<64>(D, rl, v, lane);
}

// ---- inverted diagonal blocks (once per factorization) ----
// The solves' diagonal blocks were triangular substitutions: a chain of up to 64 dependent steps
// (readlane -> fp64 fma) on one wave, ~1 us per block, on the critical path of every forward and
// backward solve -- and a Gauss-Newton step runs the solves 13 times per factorization... once.
// chol_inv_diag inverts every 64-column diagonal block after the factorization (one wave per
// block: lane c computes column c of inv(B) by column-oriented forward substitution, the block's
// entries read as wave-uniform scalar loads, 64 accumulators in registers); the solves then apply
// inv(B) (forward) or inv(B)^T (backward) as a mat-vec: independent products, 4 partial sums.
// Layout: dinv[(3 c0 + jb + col) * kSB + row] = inv(B)[row][col] for row, col < bw, B = the front's
// diagonal block at (jb, jb) (bw = min(kSB, k3 - jb)); one kSB-double column per pivot column.

// 8 consecutive doubles of LDS (16-B aligned, OFF bytes past base) into registers: four
// ds_read_b128 and one wait as inline asm with immediate offsets; `dep` is a fake operand that
// orders the loads after the arithmetic producing it.  (Left to itself the compiler issued all
// 2016 loads of a block up front and spilled 4000 registers.)
template <int OFF>
__device__ __forceinline__ void lds_ld8(uint32_t base, double (&v)[8], double& dep) {
    uint4 r0, r1, r2, r3;
    asm volatile(
        "ds_read_b128 %0, %5 offset:%6\n\t"
        "ds_read_b128 %1, %5 offset:%7\n\t"
        "ds_read_b128 %2, %5 offset:%8\n\t"
        "ds_read_b128 %3, %5 offset:%9\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "+v"(dep)
        : "v"(base), "i"(OFF), "i"(OFF + 16), "i"(OFF + 32), "i"(OFF + 48)
        : "memory");
    v[0] = __hiloint2double((int)r0.y, (int)r0.x); v[1] = __hiloint2double((int)r0.w, (int)r0.z);
    v[2] = __hiloint2double((int)r1.y, (int)r1.x); v[3] = __hiloint2double((int)r1.w, (int)r1.z);
    v[4] = __hiloint2double((int)r2.y, (int)r2.x); v[5] = __hiloint2double((int)r2.w, (int)r2.z);
    v[6] = __hiloint2double((int)r3.y, (int)r3.x); v[7] = __hiloint2double((int)r3.w, (int)r3.z);
}

// inv(B) by column-oriented forward substitution, B (column-major kSB x kSB, identity past bw) in
// LDS, lane c = column c of the inverse in registers (acc): x_J = acc_J / B_JJ, then
// acc_i -= B_iJ x_J below it, 8 rows per LDS round (entries read as broadcasts: every lane the
// same address).  Template recursion keeps every offset an immediate.
template <int J, int Q>
struct InvRows {
    static __device__ __forceinline__ void run(uint32_t base, double (&acc)[kSB], double xj) {
        if constexpr (Q < kSB / 8) {
            double v[8];
            // issued once the rows two rounds up have taken this column: two rounds in flight
            lds_ld8<(J * kSB + 8 * Q) * 8>(base, v, acc[Q >= (J >> 3) + 3 ? 8 * (Q - 2) + 7 : J]);
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[8 * Q + u] = fma(-v[u], xj, acc[8 * Q + u]);
            InvRows<J, Q + 1>::run(base, acc, xj);
        }
    }
};
template <int J>
struct InvCol {
    static __device__ __forceinline__ void run(uint32_t base, double (&acc)[kSB]) {
        if constexpr (J < kSB) {
            double v[8];
            lds_ld8<(J * kSB + (J & ~7)) * 8>(base, v, acc[J > 0 ? J - 1 : 0]);   // after x_{J-1}
            const double xj = acc[J] / v[J & 7];
            acc[J] = xj;
#pragma unroll
            for (int u = (J & 7) + 1; u < 8; ++u) acc[(J & ~7) + u] = fma(-v[u], xj, acc[(J & ~7) + u]);
            InvRows<J, (J >> 3) + 1>::run(base, acc, xj);
            InvCol<J + 1>::run(base, acc);
        }
    }
};

// one wave per diagonal block; every block padded to 64 columns (one code path)
__global__ __launch_bounds__(64) void chol_inv_diag(const Task2* __restrict__ blocks, const SnDev* __restrict__ sns,
                                                    const double* __restrict__ fronts, double* __restrict__ dinv) {
    __shared__ __attribute__((aligned(16))) double B[kSB * kSB];
    const Task2 b = blocks[blockIdx.x];   // (front, jb)
    const SnDev S = sns[b.x];
    const int m3 = 3 * (S.k + S.r), k3 = 3 * S.k, jb = b.y, bw = min(kSB, k3 - jb);
    const int lane = threadIdx.x;
    const double* F = fronts + S.front_off;
    for (int j = 0; j < kSB; ++j)   // lane = row: column j of the block, padded with the identity
        B[j * kSB + lane] = (j < bw && lane < bw) ? (lane >= j ? F[(int64_t)(jb + j) * m3 + jb + lane] : 0.0)
                                                  : (lane == j ? 1.0 : 0.0);
    __syncthreads();
    double acc[kSB];
#pragma unroll
    for (int i = 0; i < kSB; ++i) acc[i] = i == lane ? 1.0 : 0.0;
    InvCol<0>::run((uint32_t)reinterpret_cast<uintptr_t>(B), acc);
    double* out = dinv + (3 * (int64_t)S.c0 + jb) * kSB;
    if (lane < bw)
#pragma unroll
        for (int i = 0; i < kSB; ++i)
            if (i < bw) out[(int64_t)lane * kSB + i] = acc[i];
}

// the inverted block at (jb, jb) into D (ld kDL), zero past bw: as stored (forward: D(i, j) =
// inv(B)[i][j] at D[j kDL + i]) or transposed (backward: D[j kDL + i] = inv(B)[j][i])
template <bool kT_>
__device__ __forceinline__ void load_dinv(double* D, const double* dinv_front, int jb, int bw) {
    const double* src = dinv_front + (int64_t)jb * kSB;
    constexpr int kPer = kSB * kSB / kT;
    double v[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int e = threadIdx.x + kT * q, r = e % kSB, cc = e / kSB;   // src[cc * kSB + r] = inv(B)[r][cc]
        v[q] = (r < bw && cc < bw) ? src[e] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int e = threadIdx.x + kT * q, r = e % kSB, cc = e / kSB;
        if constexpr (kT_) D[r * kDL + cc] = v[q];
        else D[cc * kDL + r] = v[q];
    }
}

// one wave: v[jb + lane] <- sum_j D[j kDL + lane] v[jb + j], lane < bw (reads before the write)
__device__ __forceinline__ void apply_dinv(const double* D, double* v, int jb, int bw, int lane) {
    const int nb = chain_len(bw);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int j = 0; j < nb; j += 4) {
        const double v0 = j < bw ? v[jb + j] : 0.0, v1 = j + 1 < bw ? v[jb + j + 1] : 0.0;
        const double v2 = j + 2 < bw ? v[jb + j + 2] : 0.0, v3 = j + 3 < bw ? v[jb + j + 3] : 0.0;
        a0 = fma(D[j * kDL + lane], v0, a0);
        a1 = fma(D[(j + 1) * kDL + lane], v1, a1);
        a2 = fma(D[(j + 2) * kDL + lane], v2, a2);
        a3 = fma(D[(j + 3) * kDL + lane], v3, a3);
    }
    if (lane < bw) v[jb + lane] = (a0 + a1) + (a2 + a3);
}

// Staging of a front's L in LDS while the solve waits for its children (forward) or its parent
// (backward): every load the front's own arithmetic needs is issued before the wait, so after it
// only the handed-off values (pending row updates / the ancestors' x) travel.  The region holds
// R doubles (a launch parameter), beside the kSB x kSB diagonal-block buffer D:
//   full:  the front's pivot columns, [k3][m3] column-major exactly as in HBM (ld m3), when
//          m3 k3 <= R (its diagonal blocks are copied LDS -> D);
//   else:  the first C columns of L21 (rows k3..m3, ld r3), C a multiple of 4 (the dot products
//          keep their 4-accumulator order whichever memory a column comes from); the diagonal
//          blocks come from HBM (the first one needed is loaded before the wait).
struct Stage {
    bool full;
    int C;
};
__device__ __forceinline__ Stage stage_plan(int m3, int k3, int R) {
    if ((int64_t)m3 * k3 <= (int64_t)R) return Stage{true, k3};
    const int r3 = m3 - k3;
    const int C = r3 > 0 ? min(k3, R / r3) & ~3 : 0;
    return Stage{false, C};
}
// n doubles src -> dst, 8 loads in flight per thread
__device__ __forceinline__ void stage_copy(double* dst, const double* src, int n) {
    for (int e0 = 0; e0 < n; e0 += 8 * kT) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = e0 + threadIdx.x + kT * q;
            v[q] = e < n ? src[e] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = e0 + threadIdx.x + kT * q;
            if (e < n) dst[e] = v[q];
        }
    }
}
// L2 warm-up of the solves' unstaged reads: one load per 128-B line of every part of the front's
// L a solve reads from global memory after its wait (everything but a fully staged front and L21's
// first C columns), issued BEFORE the staging loads and retired with them -- so the front's lines
// are in this XCD's L2 when the (often tens of us long) wait ends and the diagonal blocks' and the
// column dots' loads, each a dependent round trip, hit there instead of the fabric.  The front was
// written by an earlier launch (plain loads are coherent).  Rows j, j + 16, ... of column j, and
// its last row (a 16-double step never skips a line).
constexpr int kWarm = 16;
__device__ __forceinline__ void warm_issue(const double* F, int m3, int k3, int C, double (&v)[kWarm]) {
    const int per = ((m3 + 15) >> 4) + 1, n = k3 * per;
#pragma unroll
    for (int q = 0; q < kWarm; ++q) {
        const int e = threadIdx.x + kT * q;
        v[q] = 0.0;
        if (e < n) {
            const int j = e / per;
            const int r = min(j + 16 * (e - j * per), m3 - 1);
            if (!(j < C && r >= k3)) v[q] = F[(int64_t)j * m3 + r];
        }
    }
}
// the touches retire here (an empty asm using each value: the loads cannot be dropped)
__device__ __forceinline__ void warm_retire(const double (&v)[kWarm]) {
#pragma unroll
    for (int q = 0; q < kWarm; ++q) asm volatile("" ::"v"(v[q]));
}

// the first C columns of L21 (rows k3..m3 of the front at F) -> dst [C][r3]
__device__ __forceinline__ void stage_l21(double* dst, const double* F, int m3, int k3, int C) {
    const int r3 = m3 - k3, n = C * r3;
    for (int e0 = 0; e0 < n; e0 += 8 * kT) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = e0 + threadIdx.x + kT * q;
            v[q] = e < n ? F[(int64_t)(e / r3) * m3 + k3 + e % r3] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = e0 + threadIdx.x + kT * q;
            if (e < n) dst[e] = v[q];
        }
    }
}


// z[j] -= sum_t A[j * lda + t] x[t] for j < nj, t < nt (A column-major, the dot runs down a
// column: contiguous): 16 lanes per j, so a long dot is 1/16 of the serial chain.
// Dots of at most 64 terms (a lane holds at most 4 of them: the triangular blocks' row panels,
// short L21s) are straight-line: four columns per 16-lane group in flight at once (16 loads per
// lane instead of one dependent round trip per column pass), the same fma order as the loop below.
__device__ __forceinline__ void sub_coldots(double* z, const double* A, int64_t lda, const double* x, int nj, int nt) {
    const int g = threadIdx.x >> 4, gl = threadIdx.x & 15;
    if (nt <= 64) {
        constexpr int kU = 4;
        for (int j0 = 0; j0 < nj; j0 += kU * (kT / 16)) {
            double v[kU][4];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int j = j0 + u * (kT / 16) + g;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int t = gl + 16 * q;
                    v[u][q] = (j < nj && t < nt) ? A[(int64_t)j * lda + t] : 0.0;
                }
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int j = j0 + u * (kT / 16) + g;
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
                if (gl + 48 < nt) {   // the loop's one 4-wide trip
                    a0 = fma(v[u][0], x[gl], a0);
                    a1 = fma(v[u][1], x[gl + 16], a1);
                    a2 = fma(v[u][2], x[gl + 32], a2);
                    a3 = fma(v[u][3], x[gl + 48], a3);
                } else {              // its tail
#pragma unroll
                    for (int q = 0; q < 3; ++q)
                        if (gl + 16 * q < nt) a0 = fma(v[u][q], x[gl + 16 * q], a0);
                }
                const double a = group16_sum((a0 + a1) + (a2 + a3));
                if (j < nj && gl == 0) z[j] -= a;
            }
        }
        return;
    }
    for (int j0 = 0; j0 < nj; j0 += kT / 16) {
        const int j = j0 + g;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        if (j < nj) {
            const double* Aj = A + (int64_t)j * lda;
            int t = gl;
            // 8 loads in flight per lane (the fronts come from L2/MALL: latency, not bandwidth)
#pragma unroll 2
            for (; t + 48 < nt; t += 64) {
                const double v0 = Aj[t], v1 = Aj[t + 16], v2 = Aj[t + 32], v3 = Aj[t + 48];
                a0 = fma(v0, x[t], a0);
                a1 = fma(v1, x[t + 16], a1);
                a2 = fma(v2, x[t + 32], a2);
                a3 = fma(v3, x[t + 48], a3);
            }
            for (; t < nt; t += 16) a0 = fma(Aj[t], x[t], a0);
        }
        const double a = group16_sum((a0 + a1) + (a2 + a3));
        if (j < nj && gl == 0) z[j] -= a;
    }
}

// The front's own arithmetic of the forward solve after its children's pending row updates are in:
// diagonal blocks by one wave, the rows below each block, then the pending update L21 y for the
// parent.  kFull: the front is staged in LDS at Rg (ld m3); else D holds the current diagonal block
// (the first one prestaged) and L21s the first C columns of L21.
template <bool kFull>
__device__ __forceinline__ void fwd_front(const SnDev& S, const double* F, double* Rg, double* D, const double* L21s,
                                          int C, double* rd, double* y, double* aR, double* acc, const double* dinv_f,
                                          const double* Li) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m3 = 3 * (S.k + S.r), k3 = 3 * S.k, r3 = 3 * S.r;
    const double* A = kFull ? Rg : F;   // the front's columns, ld m3
    if (Li) inv_apply_lower(Li, k3, y, D);   // y_p <- L11^-1 y_p: the whole diagonal part as one product
    for (int jb = 0; jb < (Li ? 0 : k3); jb += kSB) {
        const int bw = min(kSB, k3 - jb);
        if (jb > 0) {   // the first block was loaded before the wait
            if (dinv_f) load_dinv<false>(D, dinv_f, jb, bw);
            else if constexpr (kFull) load_diag(D, rd, Rg, m3, jb, bw);
            else load_diag(D, rd, F, m3, jb, bw);
            __syncthreads();
        }
        if (wave == 0) {
            if (dinv_f) {   // y_blk <- inv(B) y_blk
                apply_dinv(D, y, jb, bw, lane);
            } else {        // lane = row; y_j broadcast by v_readlane (uniform j)
                double yl = lane < bw ? y[jb + lane] : 0.0;
                const double rl = lane < bw ? rd[lane] : 0.0;
                yl = run_chain<true>(D, rl, yl, lane, bw);
                if (lane < bw) y[jb + lane] = yl * rl;
            }
        }
        __syncthreads();
        for (int i = jb + bw + tid; i < k3; i += kT) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            int j = 0;
#pragma unroll 2
            for (; j + 3 < bw; j += 4) {   // loads batched: a front not staged comes from L2/MALL
                const double v0 = A[(jb + j) * m3 + i], v1 = A[(jb + j + 1) * m3 + i];
                const double v2 = A[(jb + j + 2) * m3 + i], v3 = A[(jb + j + 3) * m3 + i];
                a0 = fma(v0, y[jb + j], a0);
                a1 = fma(v1, y[jb + j + 1], a1);
                a2 = fma(v2, y[jb + j + 2], a2);
                a3 = fma(v3, y[jb + j + 3], a3);
            }
            for (; j < bw; ++j) a0 = fma(A[(jb + j) * m3 + i], y[jb + j], a0);
            y[i] -= (a0 + a1) + (a2 + a3);
        }
        __syncthreads();
    }
    for (int t = tid; t < r3; t += kT) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int j = 0;
        if constexpr (kFull) {
#pragma unroll 2
            for (; j + 3 < k3; j += 4) {
                a0 = fma(Rg[j * m3 + k3 + t], y[j], a0);
                a1 = fma(Rg[(j + 1) * m3 + k3 + t], y[j + 1], a1);
                a2 = fma(Rg[(j + 2) * m3 + k3 + t], y[j + 2], a2);
                a3 = fma(Rg[(j + 3) * m3 + k3 + t], y[j + 3], a3);
            }
            for (; j < k3; ++j) a0 = fma(Rg[j * m3 + k3 + t], y[j], a0);
        } else {
            for (; j < C; j += 4) {   // C is a multiple of 4: the same accumulator order as below
                a0 = fma(L21s[j * r3 + t], y[j], a0);
                a1 = fma(L21s[(j + 1) * r3 + t], y[j + 1], a1);
                a2 = fma(L21s[(j + 2) * r3 + t], y[j + 2], a2);
                a3 = fma(L21s[(j + 3) * r3 + t], y[j + 3], a3);
            }
#pragma unroll 2
            for (; j + 3 < k3; j += 4) {
                a0 = fma(F[j * m3 + k3 + t], y[j], a0);
                a1 = fma(F[(j + 1) * m3 + k3 + t], y[j + 1], a1);
                a2 = fma(F[(j + 2) * m3 + k3 + t], y[j + 2], a2);
                a3 = fma(F[(j + 3) * m3 + k3 + t], y[j + 3], a3);
            }
            for (; j < k3; ++j) a0 = fma(F[j * m3 + k3 + t], y[j], a0);
        }
        st_agent(acc + S.acc_off + t, aR[t] + ((a0 + a1) + (a2 + a3)));
    }
}

__global__ __launch_bounds__(kT) __attribute__((amdgpu_waves_per_eu(2))) void chol_forward_dag(const int32_t* __restrict__ order, int32_t* sync,
                                                       int32_t* status, const SnDev* __restrict__ sns,
                                                       const int32_t* __restrict__ child_list,
                                                       const int32_t* __restrict__ relmap,
                                                       const double* __restrict__ fronts,
                                                       const double* __restrict__ g,
                                                       const int32_t* __restrict__ perm,
                                                       double* __restrict__ ysol, double* acc, int R,
                                                       const double* __restrict__ dinv, const int32_t* gate,
                                                       const double* __restrict__ linv) {
    extern __shared__ __attribute__((aligned(16))) double smem_fw[];
    double* sm = smem_fw + 2;   // smem_fw[0]: the claimed front (no static LDS)
    const int tid = threadIdx.x;
    if (gate_off(gate, 2)) return;
    __builtin_amdgcn_s_setprio(2);   // as chol_factor_dag
    const int s = claim_lds(order, sync, reinterpret_cast<int*>(smem_fw));
    const SnDev S = sns[s];
    const int m3 = 3 * (S.k + S.r), k3 = 3 * S.k, r3 = 3 * S.r;
    const double* F = fronts + S.front_off;
    const double* dinv_f = dinv ? dinv + 3 * (int64_t)S.c0 * kSB : nullptr;   // inverted diagonal blocks
    const double* Li = (linv && S.inv >= 0) ? linv + S.inv : nullptr;          // L11^-1
    double* D = sm;                  // kSB x kDL diagonal block (with Li: k3 doubles of scratch)
    double* Rg = D + kSB * kDL;      // staging region, R doubles (Stage)
    double* L21s = Rg;               // (not full) first C columns of L21
    double* rd = Rg + R;             // kSB reciprocals of the diagonal block's diagonal
    double* y = rd + kSB;            // k3
    double* aR = y + k3;             // r3
    const Stage P = stage_plan(m3, k3, R);
    // before the wait: the right-hand side and the front's L (earlier launches)
    for (int t = tid; t < k3; t += kT) {
        const int node = perm[S.c0 + t / 3];
        y[t] = -g[3 * node + t % 3];
    }
    for (int t = tid; t < r3; t += kT) aR[t] = 0.0;
    if (Li) {
    } else if (dinv_f) load_dinv<false>(D, dinv_f, 0, min(kSB, k3));
    else load_diag(D, rd, F, m3, 0, min(kSB, k3));
    if (P.full) {
        stage_copy(Rg, F, m3 * k3);
    } else {
        double wv[kWarm];
        if (!Li) warm_issue(F, m3, k3, P.C, wv);
        stage_l21(L21s, F, m3, k3, P.C);
        if (!Li) warm_retire(wv);
    }
    if (S.nchild > 0) {
        if (tid == 0) wait_geq_sc1(sync + 1 + s, S.nchild, status);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    for (int ci = 0; ci < S.nchild; ++ci) {
        const int c = child_list[S.child_off + ci];
        const SnDev C = sns[c];
        const int32_t* rm = relmap + C.rows_off;
        for (int t = tid; t < 3 * C.r; t += kT) {
            const int li = 3 * rm[t / 3] + t % 3;
            const double v = ld_agent(acc + C.acc_off + t);
            if (li < k3) y[li] -= v;
            else aR[li - k3] += v;
        }
        __syncthreads();
    }
    if (P.full) fwd_front<true>(S, F, Rg, D, L21s, P.C, rd, y, aR, acc, dinv_f, Li);
    else fwd_front<false>(S, F, Rg, D, L21s, P.C, rd, y, aR, acc, dinv_f, Li);
    for (int t = tid; t < k3; t += kT) ysol[3 * (int64_t)S.c0 + t] = y[t];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0 && S.parent >= 0)
        __hip_atomic_fetch_add(sync + 1 + S.parent, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// backward: L^T x = y.  A front gathers x at its row positions and subtracts L21^T x_r from y,
// segment by segment as the rows' owners publish (the highest ancestor's rows first, the parent's
// last: after the parent's signal only its own rows remain), then solves its diagonal blocks and
// publishes its own x.  Its L is staged in LDS before any wait (Stage).

// z -= L21[rows r0..r1)^T x_r[r0..r1) (scalar rows of the L21 block)
template <bool kFull>
__device__ __forceinline__ void bwd_z(const double* F, const double* Rg, const double* L21s, int C, int m3, int k3,
                                      double* z, const double* xr, int r0, int r1) {
    const int r3 = m3 - k3;
    if constexpr (kFull) {
        sub_coldots(z, Rg + k3 + r0, m3, xr + r0, k3, r1 - r0);
    } else {
        sub_coldots(z, L21s + r0, r3, xr + r0, C, r1 - r0);
        sub_coldots(z + C, F + (int64_t)C * m3 + k3 + r0, m3, xr + r0, k3 - C, r1 - r0);
    }
}

template <bool kFull>
__device__ __forceinline__ void bwd_diag(const double* F, const double* Rg, double* D, double* rd, int m3, int k3,
                                         double* z, const double* dinv_f, int s) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nblk = (k3 + kSB - 1) / kSB;
    for (int b = nblk - 1; b >= 0; --b) {
        const int jb = b * kSB, bw = min(kSB, k3 - jb);
        ST_MARK(s, 8 + b, 0);   // timing builds: per block, load / chain / column dots
        if (b != nblk - 1) {   // the last block was loaded before the wait
            if (dinv_f) load_dinv<true>(D, dinv_f, jb, bw);
            else if constexpr (kFull) load_diag(D, rd, Rg, m3, jb, bw);
            else load_diag(D, rd, F, m3, jb, bw);
            __syncthreads();
        }
        ST_MARK(s, 8 + b, 1);
        if (wave == 0) {
            if (dinv_f) {   // z_blk <- inv(B)^T z_blk
                apply_dinv(D, z, jb, bw, lane);
            } else {        // lane = row; x_j broadcast by v_readlane (uniform j): ~3 dependent ops per step
                double zl = lane < bw ? z[jb + lane] : 0.0;
                const double rl = lane < bw ? rd[lane] : 0.0;
                zl = run_chain<false>(D, rl, zl, lane, bw);
                if (lane < bw) z[jb + lane] = zl * rl;
            }
        }
        __syncthreads();
        ST_MARK(s, 8 + b, 2);
        sub_coldots(z, (kFull ? Rg : F) + jb, m3, z + jb, jb, bw);
        __syncthreads();
        ST_MARK(s, 8 + b, 3);
    }
}

template <bool kFull>
__device__ __forceinline__ void bwd_front(int s, const SnDev& S, int nseg, const SolveSeg* sg, const int32_t* rp,
                                          int32_t* sync, int32_t* status, double* xsol, const double* F, double* Rg,
                                          double* D, const double* L21s, int C, double* rd, double* z, double* xr,
                                          const double* dinv_f, const double* Li) {
    const int tid = threadIdx.x;
    const int m3 = 3 * (S.k + S.r), k3 = 3 * S.k, r3 = 3 * S.r;
    if (nseg == 0) {   // the root (no rows), or too many segments: wait for the parent, take every row
        if (S.parent >= 0) {
            if (tid == 0) wait_geq_sc1(sync + 1 + S.parent, 1, status);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        BW_MARK(s, 1);
        for (int t = tid; t < r3; t += kT) xr[t] = ld_agent(xsol + 3 * (int64_t)rp[t / 3] + t % 3);
        __syncthreads();
        bwd_z<kFull>(F, Rg, L21s, C, m3, k3, z, xr, 0, r3);
    } else {
        for (int q = nseg - 1; q >= 0; --q) {
            const SolveSeg g = sg[q];
            if (tid == 0) wait_geq_sc1(sync + 1 + g.sn, 1, status);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (q == 0) BW_MARK(s, 1);
            for (int t = 3 * g.t0 + tid; t < 3 * g.t1; t += kT) xr[t] = ld_agent(xsol + 3 * (int64_t)rp[t / 3] + t % 3);
            __syncthreads();
            bwd_z<kFull>(F, Rg, L21s, C, m3, k3, z, xr, 3 * g.t0, 3 * g.t1);
        }
    }
    __syncthreads();
    BW_MARK(s, 2);
    if (Li) inv_apply_upper(Li, k3, z, D);   // x_p <- L11^-T z_p: one product
    else bwd_diag<kFull>(F, Rg, D, rd, m3, k3, z, dinv_f, s);
}

__global__ __launch_bounds__(kT) __attribute__((amdgpu_waves_per_eu(2))) void chol_backward_dag(const int32_t* __restrict__ order, int32_t* sync,
                                                        int32_t* status, const SnDev* __restrict__ sns,
                                                        const int32_t* __restrict__ rows,
                                                        const SolveSeg* __restrict__ segs,
                                                        const double* __restrict__ fronts,
                                                        const double* __restrict__ ysol, double* xsol, int R,
                                                        int max_seg, const double* __restrict__ dinv,
                                                        const int32_t* gate, const int32_t* __restrict__ perm,
                                                        double* __restrict__ X, double* max_out,
                                                        const double* __restrict__ linv) {
    extern __shared__ __attribute__((aligned(16))) double smem_b[];
    double* sm = smem_b + 2;   // smem_b[0]: the claimed front (no static LDS)
    const int tid = threadIdx.x;
    if (gate_off(gate, 0)) return;
    __builtin_amdgcn_s_setprio(2);   // as chol_factor_dag
    const int s = claim_lds(order, sync, reinterpret_cast<int*>(smem_b));
    const SnDev S = sns[s];
    BW_MARK(s, 0);
    const int m3 = 3 * (S.k + S.r), k3 = 3 * S.k, r3 = 3 * S.r;
    const double* F = fronts + S.front_off;
    const double* dinv_f = dinv ? dinv + 3 * (int64_t)S.c0 * kSB : nullptr;   // inverted diagonal blocks
    // the inverse is valid on the gated loop's chord iterations (a refactoring iteration's is being
    // computed beside this solve) and whenever the caller passes it ungated
    const double* Li = (linv && S.inv >= 0 && (!gate || gate[1])) ? linv + S.inv : nullptr;   // L11^-1
    double* D = sm;                  // kSB x kDL diagonal block (with Li: k3 doubles of scratch)
    double* Rg = D + kSB * kDL;      // staging region, R doubles (Stage)
    double* L21s = Rg;               // (not full) first C columns of L21
    double* rd = Rg + R;             // kSB reciprocals of the diagonal block's diagonal
    double* z = rd + kSB;            // k3
    double* xr = z + k3;             // r3
    int32_t* rp = reinterpret_cast<int32_t*>(xr + r3);   // r3 / 3 row positions
    SolveSeg* sg = reinterpret_cast<SolveSeg*>(xr + r3 + ((S.r + 3) / 4) * 2);   // [kMaxSeg], 16-B aligned
    const int nseg = S.seg_n <= max_seg ? S.seg_n : 0;   // max_seg <= kMaxSeg
    const Stage P = stage_plan(m3, k3, R);
    // before any wait: y, the row positions, the segments, the front's L (all from earlier launches)
    for (int j = tid; j < k3; j += kT) z[j] = ysol[3 * (int64_t)S.c0 + j];
    for (int t = tid; t < S.r; t += kT) rp[t] = rows[S.rows_off + t];
    for (int q = tid; q < nseg; q += kT) sg[q] = segs[S.seg_off + q];
    if (!Li) {
        const int jb = ((k3 + kSB - 1) / kSB - 1) * kSB;
        if (dinv_f) load_dinv<true>(D, dinv_f, jb, k3 - jb);
        else load_diag(D, rd, F, m3, jb, k3 - jb);
    }
    if (P.full) {
        stage_copy(Rg, F, m3 * k3);
    } else {
        double wv[kWarm];
        if (!Li) warm_issue(F, m3, k3, P.C, wv);
        stage_l21(L21s, F, m3, k3, P.C);
        if (!Li) warm_retire(wv);
    }
    __syncthreads();
    if (P.full) bwd_front<true>(s, S, nseg, sg, rp, sync, status, xsol, F, Rg, D, L21s, P.C, rd, z, xr, dinv_f, Li);
    else bwd_front<false>(s, S, nseg, sg, rp, sync, status, xsol, F, Rg, D, L21s, P.C, rd, z, xr, dinv_f, Li);
    BW_MARK(s, 3);
    for (int j = tid; j < k3; j += kT) st_agent(xsol + 3 * (int64_t)S.c0 + j, z[j]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_store(sync + 1 + s, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    BW_MARK(s, 4);
    if (X) {   // the Gauss-Newton retraction of this front's nodes (retract_kernel's work), max |x|
        double m = 0.0;
        for (int j = tid; j < S.k; j += kT)
            m = fmax(m, pose_retract(X + 3 * (int64_t)perm[S.c0 + j], z[3 * j], z[3 * j + 1], z[3 * j + 2]));
        if (tid < ((S.k + 63) & ~63)) {   // the waves that own nodes
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) m = fmax(m, __shfl_down(m, off, 64));
            if ((tid & 63) == 0)
                atomicMax(reinterpret_cast<unsigned long long*>(max_out), (unsigned long long)__double_as_longlong(m));
        }
    }
}

// ---- fused factorization + forward solve: ONE launch, fronts as a DAG ----
// One 512-thread workgroup per front, claimed in topological order (as the solves above).  A
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
// Hand-off (Guideline 16, R1): everything another workgroup reads -- the update matrix (columns
// >= k3) and the pending row updates -- is stored write-through (sc1, agent-scope relaxed stores)
// and read back with sc1 loads; every storing wave drains, the workgroup synchronises, ONE lane
// adds to the parent's counter; the consumer polls relaxed, then one agent-scope acquire.
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

// A front of more than kSmall rows is factored by a TEAM of G workgroups (G consecutive tickets).
// Its columns are cut into tiles of kFNB: pivot tiles [kFNB t, min(kFNB t + kFNB, k3)), then update
// tiles from k3; tile t belongs to member t mod G, and only its owner ever writes it (plain stores).
// Per pivot panel p the owner -- who has already applied panels 0..p-1 to its tile -- factors it
// (POTRF of the top block by one wave, TRSM of the rows below, one row per thread), publishes it
// write-through (sc1) and raises the front's panel flag; every member with tiles right of p loads
// the panel (sc1) into LDS and applies the rank-w update to its own tiles (4x4 register tiles).
// Member 0 also carries the right-hand side (forward solve folded in, as in small_front).  The
// children's update matrices are added into the owners' columns in child order; at the end every
// member republishes its update tiles write-through and adds 1 to the parent's counter (which
// waits for the sum of its children's team sizes).
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
            ST_MARK(s, q, wave);
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
struct SelPick { int64_t off; int32_t ld, pad; };
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

struct CholDev {
    // (first among the resources, so destroyed last: the L11^-1 stream of the gated loop)
    DevStream aux;
    dpg_chol_opts opts;   // the context's solver options at creation
    dpg_chol_sym sym;
    // the plan of `sym` (dpg_chol_plan.cpp): host arrays, sizes and launch parameters.  A plan and
    // its upload may run on different threads, one after the other; dpg_chol_plan_blocks fills its
    // H-block buckets beside the next analysis's derivation.
    CholPlan plan;
    // the plan's arrays on the device: non-owning views into `arena`, set by chol_upload
    SnDev* sns = nullptr;
    OEnt* omap = nullptr;
    int32_t* child_list = nullptr;
    int32_t* relmap = nullptr;
    int32_t* rows = nullptr;
    int32_t* perm = nullptr;
    int32_t* pos = nullptr;
    int32_t* order_fwd = nullptr;      // forward solve: fronts in the tickets' order
    int32_t* order_fac = nullptr;      // fused factorization tickets (front * 64 + member)
    int32_t* order_bwd = nullptr;
    FTask* ftasks = nullptr;           // large fronts: per-tile assembly lists
    FChild* fchild = nullptr;
    SolveSeg* segs = nullptr;
    Task2* dblocks = nullptr;          // (front, jb) of every diagonal block
    Task2* inv_tasks = nullptr;        // chol_inv_l11: (front, first column) per workgroup
    AsmTask* asm_tasks = nullptr;      // level path
    AsmChild* asm_child = nullptr;
    Task2* panel_tasks = nullptr;
    Task4* upd_tasks = nullptr;
    // values.  The buffers are kept between rebuilds of the same solver (an incremental graph
    // re-derives its structures every update): re-allocated only when one must grow, by 1.5x at least
    DevBuf<double> fronts, acc, ysol, xsol;
    DevBuf<int32_t> status;
    DevBuf<double> dinv;               // inverted diagonal blocks of the solves ([3n][kSB])
    DevBuf<double> linv;               // L11^-1 of the large fronts (SnDev.inv offsets)
    DevBuf<int32_t> sync;              // plan.sync_bytes of counters and flags, zeroed per solve (SyncWords)
    // L11^-1 (chol_inv_l11): valid for the last factorization (inv_valid: computed by an ungated
    // solve); the gated loop computes it on `aux` beside each refactoring iteration's backward solve
    // and its chord iterations wait for it (ev_inv of the previous iteration)
    bool inv_valid = false;
    bool keep_inv = false;   // ungated solves compute L11^-1 after their backward solve (for dpg_chol_resolve)
    DevEvent ev_fac, ev_inv[2];
    int inv_par = 0;
    double t_build[2] = {0, 0};   // last chol_build: host structures, uploads (ms)
    PinBuf<char> stage;           // pinned staging buffer of the uploads
    DevBuf<char> arena;           // device: every structure array above (sns .. upd_tasks), one copy
    // partial refactorization (dpg_chol_track_factor): `fac_sym` is the analysis the values in
    // `fronts` were factored under (valid while fac_valid and fronts == fac_ptr), fac_G its team
    // sizes; sym_is_fac: the current analysis is that one (it moves to fac_sym with the next plan)
    bool track = false, fac_valid = false, sym_is_fac = false, fac_db = false;
    double* fac_ptr = nullptr;         // fronts, y and the pending updates of that factorization
    double* fac_ysol = nullptr;        // (identities to compare with, not owned)
    double* fac_acc = nullptr;
    dpg_chol_sym fac_sym;
    std::vector<int32_t> fac_G;   // (the current analysis's: plan.cur_G)
    std::vector<uint8_t> h_keep;
    std::vector<int32_t> h_old;
    std::vector<int64_t> h_runs;
    DevBuf<double> scratch;       // the moved fronts between the gather and the scatter
    PinBuf<char> pstage;          // pinned: keep flags + runs, one copy up
    DevBuf<char> dpart;
    DevEvent pev;                 // after that copy (the staging buffer's next rewrite waits for it)
    bool pev_set = false;
    int64_t pstats[4] = {0, 0, 0, 0};   // last solve: fronts refactored, kept, doubles moved, host ns of the pick
    // selected inverse (dpg_chol_selinv): nothing here is allocated or built before the first
    // request.  `sel` has the fronts' layout; `sel_work` holds [Z; Y] of the fronts too large for
    // LDS (sel_woff); sel_list = level_list on the device.  The lists belong to the analysis
    // uploaded as number build_gen (sel_gen: the one they were built for).
    bool has_factor = false;      // `fronts` holds a factorization under the current analysis
    int64_t build_gen = 0, sel_gen = -1;
    DevBuf<double> sel, sel_work, sel_out;
    DevBuf<char> sel_lists;       // [int64 woff[ns] | int32 list[ns]]
    DevBuf<SelPick> sel_picks;
    std::vector<size_t> sel_lds;  // per level: dynamic LDS bytes of its launch
    std::vector<SelPick> h_picks;
    std::vector<DevEvent> sel_ev;
    // joint marginals (dpg_chol_joint): its own plan and buffers, allocated by the first request and
    // regrown only when a request needs more; nothing above is written
    JointPlan jplan;
    DevBuf<double> jt_w;          // the compact W buffer (the queries' slices)
    DevBuf<double> jt_work;       // the path solve's vectors when they do not fit LDS
    DevBuf<double> jt_out;
    DevBuf<char> jt_lists;        // [PathPair pairs | PathQuery queries]
    DevEvent jt_ev[3];
};

// a new analysis in; *S gets back one whose buffers the caller reuses.  With tracking, the analysis
// of the last factorization moves to fac_sym instead (the partial refactorization compares with it)
void take_sym(CholDev* c, dpg_chol_sym* S) {
    c->has_factor = false;   // (the values in fronts belong to the analysis leaving)
    if (c->track && c->sym_is_fac) {
        std::swap(c->fac_sym, c->sym);
        c->fac_G.swap(c->plan.cur_G);
        c->sym_is_fac = false;
    }
    std::swap(c->sym, *S);
}

}  // namespace

extern "C" void dpg_chol_destroy(void* h) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    if (!c) return;
    if (c->aux.s) (void)hipStreamSynchronize(c->aux.s);
    delete c;
}

namespace {
// Device structures of the factorization for the symbolic analysis in c->sym (reusing c's buffers).
int chol_build(CholDev* c, int64_t n, const int32_t* pair_lo, const int32_t* pair_hi, int64_t n_pairs);
}  // namespace

extern "C" int dpg_chol_create(void** out, int64_t n, const int32_t* pair_lo, const int32_t* pair_hi,
                               int64_t n_pairs, const dpg_chol_opts* opts) {
    *out = nullptr;
    CholDev* c = new CholDev();
    if (opts) c->opts = *opts;
    if (dpg_chol_symbolic(n, pair_lo, pair_hi, n_pairs, &c->opts, &c->sym)) {
        delete c;
        return DPG_ERR_NUMERIC;
    }
    const int rc = chol_build(c, n, pair_lo, pair_hi, n_pairs);
    if (rc) { dpg_chol_destroy(c); return rc; }
    *out = c;
    return DPG_OK;
}

// The same from a given symbolic analysis; *h is reused (its buffers grow when needed) or created.
int dpg_chol_create_sym(void** h, int64_t n, const int32_t* pair_lo, const int32_t* pair_hi, int64_t n_pairs,
                        dpg_chol_sym* S, const dpg_chol_opts* opts) {
    CholDev* c = *h ? reinterpret_cast<CholDev*>(*h) : new CholDev();
    if (opts) c->opts = *opts;
    take_sym(c, S);   // *S gets an earlier analysis (its buffers are reused by the next derive)
    const int rc = chol_build(c, n, pair_lo, pair_hi, n_pairs);
    if (rc) { dpg_chol_destroy(c); *h = nullptr; return rc; }
    *h = c;
    return DPG_OK;
}

namespace {
// The structure arrays are packed into one pinned staging buffer and go up in ONE asynchronous
// copy into one device arena (the pointers of c point into it); one synchronisation at the end.
int chol_upload(CholDev* c) {
    const dpg_chol_sym& S = c->sym;
    const CholPlan& H = c->plan;
    const int64_t n = H.n;
    ++c->build_gen;   // (the selected inverse's lists follow the analysis: rebuilt on its next request)
    c->has_factor = false;
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    struct Piece { void** d; const void* h; size_t bytes; };
    Piece pieces[24];
    int np = 0;
    auto add = [&](auto** d, const auto& h) {
        using T = typename std::remove_reference<decltype(h)>::type::value_type;
        pieces[np++] = Piece{reinterpret_cast<void**>(d), h.data(), h.size() * sizeof(T)};
    };
    add(&c->sns, H.sns);
    add(&c->omap, H.omap);
    add(&c->child_list, S.child_list);
    add(&c->relmap, S.relmap);
    add(&c->rows, S.sn_rows);
    add(&c->perm, S.perm);
    add(&c->pos, S.pos);
    add(&c->order_fwd, H.fo);
    add(&c->order_fac, H.order_fac);
    add(&c->ftasks, H.ftasks);
    add(&c->fchild, H.fchild);
    add(&c->order_bwd, H.bwd);
    add(&c->segs, H.segs);
    add(&c->dblocks, H.dblocks);
    add(&c->inv_tasks, H.inv_t);
    if (!H.fused) {
        add(&c->asm_tasks, H.asm_t);
        add(&c->asm_child, H.asm_c);
        add(&c->panel_tasks, H.panel_t);
        add(&c->upd_tasks, H.upd_t);
    }
    size_t total = 0;
    for (int i = 0; i < np; ++i) total += al(std::max<size_t>(pieces[i].bytes, 1));
    if (c->stage.reserve_amortised(total) || c->arena.reserve_amortised(total)) return DPG_ERR_HIP;
    size_t off = 0;
    for (int i = 0; i < np; ++i) {
        if (pieces[i].bytes) memcpy(c->stage.p + off, pieces[i].h, pieces[i].bytes);
        *pieces[i].d = c->arena.p + off;
        off += al(std::max<size_t>(pieces[i].bytes, 1));
    }
    int rc = hipMemcpyAsync(c->arena.p, c->stage.p, total, hipMemcpyHostToDevice, nullptr) != hipSuccess;
    // a re-allocated front, y or pending-update buffer has lost the tracked factorization (a new
    // allocation may come back at the old address: the capacities tell)
    const size_t cap0[3] = {c->fronts.cap, c->acc.cap, c->ysol.cap};
    rc |= c->sync.reserve_amortised(H.sync_bytes / sizeof(int32_t));
    rc |= c->fronts.reserve_amortised((size_t)S.front_off[(size_t)S.ns]);
    rc |= c->acc.reserve_amortised((size_t)H.acc_total);
    rc |= c->ysol.reserve_amortised((size_t)(3 * n));
    if (rc || cap0[0] != c->fronts.cap || cap0[1] != c->acc.cap || cap0[2] != c->ysol.cap) c->fac_valid = false;
    rc |= c->xsol.reserve_amortised((size_t)(3 * n));
    rc |= c->status.reserve_amortised(1);
    rc |= c->dinv.reserve_amortised((size_t)(3 * n) * kSB);
    rc |= c->linv.reserve_amortised((size_t)std::max<int64_t>(H.linv_total, 1));
    if (!rc) rc |= hipMemsetAsync(c->status.p, 0, sizeof(int32_t), nullptr) != hipSuccess;
    // the staging buffer is reused by the next build: wait for the copy (always, even after an error)
    rc |= hipStreamSynchronize(nullptr) != hipSuccess;
    return rc ? DPG_ERR_HIP : DPG_OK;
}

// (a plan and its upload may be split: dpg_chol_create_sym_plan / _upload, possibly on two threads
// one after the other)
int chol_build_plan(CholDev* c, int64_t n, const int32_t* pair_lo, const int32_t* pair_hi, int64_t n_pairs) {
    const double t_b0 = now_ms();
    const int rc = dpg_chol_plan_build(c->plan, c->sym, c->opts, c->track, n, pair_lo, pair_hi, n_pairs);
    c->t_build[0] = now_ms() - t_b0;
    return rc;
}
int chol_build_upload(CholDev* c) {
    const double t_b1 = now_ms();
    const int rc = chol_upload(c);
    c->t_build[1] = now_ms() - t_b1;
    return rc;
}
int chol_build(CholDev* c, int64_t n, const int32_t* pair_lo, const int32_t* pair_hi, int64_t n_pairs) {
    const int rc = chol_build_plan(c, n, pair_lo, pair_hi, n_pairs);
    return rc ? rc : chol_build_upload(c);
}
}  // namespace

// dpg_chol_create_sym in two halves: the plan (host only: no device call, so it may run while the
// caller's stream still works, on any thread) and the upload of what it planned (nothing between)
int dpg_chol_create_sym_plan(void** h, int64_t n, const int32_t* pair_lo, const int32_t* pair_hi, int64_t n_pairs,
                             dpg_chol_sym* S, const dpg_chol_opts* opts) {
    CholDev* c = *h ? reinterpret_cast<CholDev*>(*h) : new CholDev();
    if (opts) c->opts = *opts;
    take_sym(c, S);
    const int rc = chol_build_plan(c, n, pair_lo, pair_hi, n_pairs);
    if (rc) { dpg_chol_destroy(c); *h = nullptr; return rc; }
    *h = c;
    return DPG_OK;
}
// the plan's first stage ahead of the plan (pos / perm: the ordering the plan's analysis will
// carry); creates the solver object when *h is NULL.  Host only; not concurrently with a plan or an
// upload of the same object.
int dpg_chol_plan_blocks(void** h, int64_t n, const int32_t* pos, const int32_t* perm, const int32_t* pair_lo,
                         const int32_t* pair_hi, int64_t n_pairs) {
    if (!h || n <= 0 || !pos || !perm || n_pairs < 0 || (n_pairs > 0 && (!pair_lo || !pair_hi))) return DPG_ERR_ARG;
    CholDev* c = *h ? reinterpret_cast<CholDev*>(*h) : new CholDev();
    *h = c;
    dpg_chol_plan_prebucket(c->plan, n, pos, perm, pair_lo, pair_hi, n_pairs);
    return DPG_OK;
}
// drop prebuilt H-block buckets (their ordering was not the one the next plan will carry: the
// derivation they were built beside failed)
void dpg_chol_blocks_invalidate(void* h) {
    if (h) reinterpret_cast<CholDev*>(h)->plan.blocks_ready = false;
}
int dpg_chol_create_sym_upload(void** h) {
    CholDev* c = reinterpret_cast<CholDev*>(*h);
    if (!c) return DPG_ERR_STATE;
    const int rc = chol_build_upload(c);
    if (rc) { dpg_chol_destroy(c); *h = nullptr; }
    return rc;
}

int dpg_chol_fused(void* h) { return h && reinterpret_cast<const CholDev*>(h)->plan.fused ? 1 : 0; }

void dpg_chol_build_times(void* h, double out[2]) {
    const CholDev* c = reinterpret_cast<const CholDev*>(h);
    out[0] = c ? c->t_build[0] : 0.0;
    out[1] = c ? c->t_build[1] : 0.0;
}

// ---- one launch site per solver kernel ----
// The sync words of one solve (plan.sync_bytes, zeroed before the factorization, or before the
// forward solve where it runs alone), ns = the number of fronts:
//   [0]                    ticket of the factorization / the forward solve
//   [1, 1 + ns)            children-done counters of the same
//   [1 + ns, 1 + 2 ns)     panel flags of the large fronts
//   [1 + 2 ns]             ticket of the backward solve
//   [2 + 2 ns, 2 + 3 ns)   its done flags
//   [2 + 3 ns, ..)         pivot-tile hand-off flags, one per large-front tile
// Each kernel takes the base of its part (chol_factor_dag the whole array), and these helpers are
// the only places that know the offsets.  The level path's backward solve used to take its part at
// 1 + ns -- inside the panel flags, which that path never uses; it now takes 1 + 2 ns like every
// other caller: the only launch argument that differs from the hand-written launches these
// helpers replaced.
//
// gate: the pipelined loop's (gate_off); keep: the partial refactorization's per-front flags; di /
// li: inverted diagonal blocks / L11^-1 for the solves' diagonal part; X, max_out: the backward
// solve retracts the poses as it goes.

// fused factorization + forward solve of hb's system (its right-hand side follows its blocks)
static void launch_factor(CholDev* c, hipStream_t st, const double* hb, const int32_t* gate, const uint8_t* keep) {
    const CholPlan& P = c->plan;
    hipLaunchKernelGGL(chol_factor_dag, dim3((unsigned)P.n_tickets), dim3(kFT), P.lds_fused, st, c->order_fac, c->sync.p,
                       c->status.p, c->sns, c->omap, c->relmap, c->child_list, c->ftasks, c->fchild, hb, hb + 9 * P.nnzb_upper,
                       c->perm, c->fronts.p, c->ysol.p, c->acc.p, c->sym.ns, P.fused_db ? 1 : 0, gate, keep);
}

static void launch_forward(CholDev* c, hipStream_t st, const double* hb, const double* di, const int32_t* gate,
                           const double* li) {
    const CholPlan& P = c->plan;
    hipLaunchKernelGGL(chol_forward_dag, dim3(c->sym.ns), dim3(kT), P.lds_solve_max, st, c->order_fwd, c->sync.p, c->status.p,
                       c->sns, c->child_list, c->relmap, c->fronts.p, hb + 9 * P.nnzb_upper, c->perm, c->ysol.p, c->acc.p,
                       P.solve_stage, di, gate, li);
}

static void launch_backward(CholDev* c, hipStream_t st, const double* di, const int32_t* gate, double* X, double* max_out,
                            const double* li) {
    const CholPlan& P = c->plan;
    const int32_t ns = c->sym.ns;
    hipLaunchKernelGGL(chol_backward_dag, dim3(ns), dim3(kT), P.lds_solve_max, st, c->order_bwd, c->sync.p + 1 + 2 * ns,
                       c->status.p, c->sns, c->rows, c->segs, c->fronts.p, c->ysol.p, c->xsol.p, P.solve_stage, P.solve_maxseg, di, gate,
                       X ? c->perm : nullptr, X, max_out, li);
}

// the solves' inverted diagonal blocks from the fronts just factored (opts.solve_dinv); returns
// what the solves take as `di`
static const double* launch_inv_diag(CholDev* c, hipStream_t st) {
    const CholPlan& P = c->plan;
    if (P.use_dinv && P.n_dblocks > 0)
        hipLaunchKernelGGL(chol_inv_diag, dim3((unsigned)P.n_dblocks), dim3(64), 0, st, c->dblocks, c->sns, c->fronts.p, c->dinv.p);
    return P.use_dinv ? c->dinv.p : nullptr;
}

// L11^-1 of the large fronts from the fronts just factored (gate: the pipelined loop's, refactoring
// iterations only)
static void launch_inv(CholDev* c, hipStream_t st, const int32_t* gate) {
    const CholPlan& P = c->plan;
    if (P.n_inv_tasks > 0)
        hipLaunchKernelGGL(chol_inv_l11, dim3((unsigned)P.n_inv_tasks), dim3(kInvThreads), P.lds_inv, st, c->inv_tasks, c->sns,
                           c->fronts.p, c->linv.p, gate);
}

// the level-synchronous factorization: per level, assembly tiles, then panel + update steps
static void launch_levels(CholDev* c, hipStream_t st, const double* hb) {
    int pid = 0;
    for (const CholPlan::Level& L : c->plan.levels) {
        hipLaunchKernelGGL(chol_assemble, dim3(L.asm_cnt), dim3(kT), L.lds_asm, st, c->asm_tasks + L.asm_off,
                           c->asm_child, c->sns, c->omap, hb, c->relmap, c->fronts.p, pid++);
        for (const CholPlan::Step& p : L.steps) {
            const Task2* pt = c->panel_tasks + p.panel_off;
            if (p.rpt == 1) hipLaunchKernelGGL(chol_panel<kT>, dim3(p.panel_cnt), dim3(kT), 0, st, pt, c->sns, c->fronts.p, c->status.p, pid++);
            else if (p.rpt == 2) hipLaunchKernelGGL(chol_panel<2 * kT>, dim3(p.panel_cnt), dim3(2 * kT), 0, st, pt, c->sns, c->fronts.p, c->status.p, pid++);
            else hipLaunchKernelGGL(chol_panel<4 * kT>, dim3(p.panel_cnt), dim3(4 * kT), 0, st, pt, c->sns, c->fronts.p, c->status.p, pid++);
            if (p.upd_cnt > 0)
                hipLaunchKernelGGL(chol_update, dim3(p.upd_cnt), dim3(kT), 0, st, c->upd_tasks + p.upd_off, c->sns, c->fronts.p, pid++);
        }
    }
}

// the values in fronts now belong to the current analysis
static void note_factored(CholDev* c, int64_t refactored, int64_t kept, int64_t moved, int64_t pick_ns = 0) {
    c->pstats[0] = refactored;
    c->pstats[1] = kept;
    c->pstats[2] = moved;
    c->pstats[3] = pick_ns;
    c->has_factor = true;
    if (!c->track) return;
    c->fac_valid = true;
    c->fac_ptr = c->fronts.p;
    c->fac_ysol = c->ysol.p;
    c->fac_acc = c->acc.p;
    c->sym_is_fac = true;
    c->fac_db = c->plan.fused_db;
}

extern "C" int dpg_chol_solve(void* h, const double* hb, void* stream) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    const CholPlan& P = c->plan;
    note_factored(c, c->sym.ns, 0, 0);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(c->status.p, 0, sizeof(int32_t), st) != hipSuccess) return DPG_ERR_HIP;
    if (P.fused) {
        if (hipMemsetAsync(c->sync.p, 0, P.sync_bytes, st) != hipSuccess) return DPG_ERR_HIP;
        launch_factor(c, st, hb, nullptr, nullptr);
    } else {
        launch_levels(c, st, hb);
        if (hipMemsetAsync(c->sync.p, 0, P.sync_bytes, st) != hipSuccess) return DPG_ERR_HIP;
    }
    const double* di = launch_inv_diag(c, st);
    if (!P.fused) launch_forward(c, st, hb, di, nullptr, nullptr);
    launch_backward(c, st, di, nullptr, nullptr, nullptr, nullptr);
    // the inverse after the backward (which, as a refactoring iteration of the gated loop, chains):
    // the chord steps of dpg_chol_resolve then do the same arithmetic as the gated loop's
    c->inv_valid = c->keep_inv && P.n_inv_tasks > 0;
    if (c->inv_valid) launch_inv(c, st, nullptr);
    return hipGetLastError() == hipSuccess ? DPG_OK : DPG_ERR_HIP;
}

extern "C" void dpg_chol_track_factor(void* h, int on) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    if (!c || c->track == (on != 0)) return;
    c->track = on != 0;
    c->fac_valid = false;
    c->sym_is_fac = false;
    c->plan.cur_G.clear();   // the current analysis was planned untracked: its team sizes are unknown
}
extern "C" void dpg_chol_forget_factor(void* h) {
    if (!h) return;
    reinterpret_cast<CholDev*>(h)->fac_valid = false;
    reinterpret_cast<CholDev*>(h)->has_factor = false;
}
extern "C" void dpg_chol_partial_stats(void* h, int64_t out[4]) {
    const CholDev* c = reinterpret_cast<const CholDev*>(h);
    for (int k = 0; k < 4; ++k) out[k] = c ? c->pstats[k] : 0;
}

// ISAM2's partial re-elimination (isam_->update, dpg_slam.cc:320, re-eliminates only the cliques
// the new factors touch and their ancestors), as a multifrontal refactorization that keeps every
// front whose values cannot have changed since the tracked factorization:
//   * the same columns (same first column, same count: positions are stable between reorders, the
//     caller checks the order is unchanged -- here: the old order is a prefix of the new), the same
//     rows, the same children (by first column, in order: the extend-add order), the same team
//     size and panel buffering (the arithmetic order of the factorization kernel);
//   * no dirty node's column in it (its H blocks are then the same sums of the same factors at the
//     same linearization point: the caller's contract);
//   * no dirty front below it (its children's update matrices are unchanged).
// The forward solve folded into the factorization keeps its values too: a kept front's nodes have
// the same gradient (no new factor on them, same theta) and its children are kept, so its part of y
// (at its column positions: unchanged between reorders) and its pending row updates for the parent
// are what a full refactorization would compute again.  A kept front the new layout moved -- its
// values and its pending updates -- goes through the scratch buffer (gather, scatter), then the
// factorization runs with the kept fronts only signalling their parents, then the backward solve
// over every front.  The result is bit-identical to dpg_chol_solve's.
extern "C" int dpg_chol_solve_partial(void* h, const double* hb, const int32_t* dirty_nodes, int64_t n_dirty,
                                      void* stream) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    const dpg_chol_sym& S = c->sym;
    const dpg_chol_sym& O = c->fac_sym;
    const CholPlan& P = c->plan;
    const bool usable = c->track && c->fac_valid && !c->sym_is_fac && c->fac_ptr == c->fronts.p &&
                        c->fac_ysol == c->ysol.p && c->fac_acc == c->acc.p && P.fused &&
                        !(P.use_dinv && P.n_dblocks > 0) && c->fac_db == P.fused_db && O.ns > 0 && O.n <= S.n &&
                        (int64_t)c->fac_G.size() == (int64_t)O.ns && (int64_t)P.cur_G.size() == (int64_t)S.ns &&
                        std::equal(O.perm.begin(), O.perm.end(), S.perm.begin());
    if (!usable) return dpg_chol_solve(h, hb, stream);
    const double t_pick = now_ms();
    const int32_t ns = S.ns;
    std::vector<uint8_t>& keep = c->h_keep;
    std::vector<int32_t>& old = c->h_old;
    keep.assign((size_t)ns, 1);
    old.assign((size_t)ns, -1);
    for (int64_t q = 0; q < n_dirty; ++q) {
        const int32_t v = dirty_nodes[q];
        if (v < 0 || v >= S.n) return dpg_chol_solve(h, hb, stream);
        keep[(size_t)S.sn_of[(size_t)S.pos[(size_t)v]]] = 0;
    }
    int64_t kept = 0;
    for (int32_t sn = 0; sn < ns; ++sn) {   // children before parents (a parent's first column is later)
        if (keep[(size_t)sn]) {
            const int32_t c0 = S.sn_c0[(size_t)sn], c1 = S.sn_c0[(size_t)sn + 1];
            bool same = c1 <= O.n;
            int32_t os = -1;
            if (same) {
                os = O.sn_of[(size_t)c0];
                same = O.sn_c0[(size_t)os] == c0 && O.sn_c0[(size_t)os + 1] == c1 && c->fac_G[(size_t)os] == P.cur_G[(size_t)sn];
            }
            if (same) {
                const int64_t r0 = S.sn_rows_ptr[(size_t)sn], r1 = S.sn_rows_ptr[(size_t)sn + 1];
                const int64_t q0 = O.sn_rows_ptr[(size_t)os], q1 = O.sn_rows_ptr[(size_t)os + 1];
                same = r1 - r0 == q1 - q0 && std::equal(S.sn_rows.begin() + r0, S.sn_rows.begin() + r1, O.sn_rows.begin() + q0);
            }
            if (same) {
                const int64_t a0 = S.child_ptr[(size_t)sn], a1 = S.child_ptr[(size_t)sn + 1];
                const int64_t b0 = O.child_ptr[(size_t)os], b1 = O.child_ptr[(size_t)os + 1];
                same = a1 - a0 == b1 - b0;
                for (int64_t t = 0; same && t < a1 - a0; ++t)
                    same = S.sn_c0[(size_t)S.child_list[(size_t)(a0 + t)]] == O.sn_c0[(size_t)O.child_list[(size_t)(b0 + t)]];
            }
            if (same) {
                old[(size_t)sn] = os;
                ++kept;
            } else {
                keep[(size_t)sn] = 0;
            }
        }
        if (!keep[(size_t)sn] && S.sn_parent[(size_t)sn] >= 0) keep[(size_t)S.sn_parent[(size_t)sn]] = 0;
    }
    if (kept == 0) return dpg_chol_solve(h, hb, stream);
    // runs of kept fronts the layout moved: gather {old, scratch}, scatter {scratch, new}; the
    // pending updates of front s sit at 3 sn_rows_ptr[s] (the plan's acc_off)
    std::vector<int64_t>& runs = c->h_runs;
    runs.clear();
    int64_t moved = 0, max_run = 0;
    auto add_run = [&](int64_t src, int64_t dst, int64_t len, int64_t buf) {
        if (src == dst || len == 0) return;
        const size_t nr = runs.size();
        if (nr >= 4 && runs[nr - 1] == buf && runs[nr - 4] + runs[nr - 2] == src && runs[nr - 3] + runs[nr - 2] == dst) {
            runs[nr - 2] += len;
        } else {
            runs.push_back(src);
            runs.push_back(dst);
            runs.push_back(len);
            runs.push_back(buf);
        }
        max_run = std::max(max_run, runs[runs.size() - 2]);
        moved += len;
    };
    for (int32_t sn = 0; sn < ns; ++sn)
        if (keep[(size_t)sn])
            add_run(O.front_off[(size_t)old[(size_t)sn]], S.front_off[(size_t)sn],
                    S.front_off[(size_t)sn + 1] - S.front_off[(size_t)sn], 0);
    for (int32_t sn = 0; sn < ns; ++sn)
        if (keep[(size_t)sn])
            add_run(3 * O.sn_rows_ptr[(size_t)old[(size_t)sn]], 3 * S.sn_rows_ptr[(size_t)sn],
                    3 * (S.sn_rows_ptr[(size_t)sn + 1] - S.sn_rows_ptr[(size_t)sn]), 1);
    const int64_t nruns = (int64_t)runs.size() / 4;
    if (nruns > 65535) return dpg_chol_solve(h, hb, stream);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // keep flags + gather runs + scatter runs: one pinned buffer, one copy up
    const size_t keep_bytes = ((size_t)ns + 15) & ~size_t(15);
    const size_t run_bytes = sizeof(int64_t) * 4 * (size_t)nruns;
    const size_t bytes = keep_bytes + 2 * run_bytes;
    if (c->pev_set && hipEventSynchronize(c->pev.e) != hipSuccess) return DPG_ERR_HIP;
    if (c->pstage.reserve_amortised(bytes) || c->dpart.reserve_amortised(bytes) ||
        (moved > 0 && c->scratch.reserve_amortised((size_t)moved)))
        return DPG_ERR_HIP;
    memcpy(c->pstage.p, keep.data(), (size_t)ns);
    int64_t* gat = reinterpret_cast<int64_t*>(c->pstage.p + keep_bytes);
    int64_t* sca = gat + 4 * nruns;
    for (int64_t r = 0, off = 0; r < nruns; ++r) {
        const int64_t* q = runs.data() + 4 * r;
        const int64_t g4[4] = {q[0], off, q[2], q[3]}, s4[4] = {off, q[1], q[2], q[3]};
        std::copy(g4, g4 + 4, gat + 4 * r);
        std::copy(s4, s4 + 4, sca + 4 * r);
        off += q[2];
    }
    if (c->pev.ensure(hipEventDisableTiming)) return DPG_ERR_HIP;
    if (hipMemcpyAsync(c->dpart.p, c->pstage.p, bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipEventRecord(c->pev.e, st) != hipSuccess)
        return DPG_ERR_HIP;
    c->pev_set = true;
    const uint8_t* keep_dev = reinterpret_cast<const uint8_t*>(c->dpart.p);
    const int64_t* gat_dev = reinterpret_cast<const int64_t*>(c->dpart.p + keep_bytes);
    const int64_t* sca_dev = gat_dev + 4 * nruns;
    if (nruns > 0) {
        const unsigned gx = (unsigned)std::min<int64_t>(64, std::max<int64_t>(1, (max_run + 2047) / 2048));
        hipLaunchKernelGGL(chol_copy_runs, dim3(gx, (unsigned)nruns), dim3(256), 0, st, c->fronts.p, c->acc.p, c->scratch.p,
                           c->scratch.p, gat_dev);
        hipLaunchKernelGGL(chol_copy_runs, dim3(gx, (unsigned)nruns), dim3(256), 0, st, c->scratch.p, c->scratch.p, c->fronts.p,
                           c->acc.p, sca_dev);
    }
    if (hipMemsetAsync(c->status.p, 0, sizeof(int32_t), st) != hipSuccess ||
        hipMemsetAsync(c->sync.p, 0, P.sync_bytes, st) != hipSuccess)
        return DPG_ERR_HIP;
    launch_factor(c, st, hb, nullptr, keep_dev);
    launch_backward(c, st, nullptr, nullptr, nullptr, nullptr, nullptr);
    note_factored(c, ns - kept, kept, moved, (int64_t)((now_ms() - t_pick) * 1e6));
    c->inv_valid = false;
    return hipGetLastError() == hipSuccess ? DPG_OK : DPG_ERR_HIP;
}

// forward + backward solves with the fronts of the last factorization (the right-hand side from hb)
extern "C" int dpg_chol_resolve(void* h, const double* hb, void* stream) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(c->sync.p, 0, c->plan.sync_bytes, st) != hipSuccess) return DPG_ERR_HIP;
    const double* di = c->plan.use_dinv ? c->dinv.p : nullptr;   // inverted by the factorization's dpg_chol_solve
    const double* li = c->inv_valid ? c->linv.p : nullptr;
    launch_forward(c, st, hb, di, nullptr, li);
    launch_backward(c, st, di, nullptr, nullptr, nullptr, li);
    return hipGetLastError() == hipSuccess ? DPG_OK : DPG_ERR_HIP;
}

// one Gauss-Newton iteration's solve with the path chosen on the device (gate, see gate_off):
// the fused factorization + forward solve, or the forward solve with the last factor, then the
// backward solve.  Only the fused plan without inverted diagonal blocks (dpg_chol_gated_ok).
extern "C" int dpg_chol_gated_ok(void* h) {
    const CholDev* c = reinterpret_cast<const CholDev*>(h);
    return c && c->plan.fused && !(c->plan.use_dinv && c->plan.n_dblocks > 0) ? 1 : 0;
}

extern "C" void dpg_chol_sync_dev(void* h, int32_t** sync, int64_t* n_words) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    *sync = c->sync.p;
    *n_words = (int64_t)(c->plan.sync_bytes / sizeof(int32_t));
}

// prezeroed: the caller's previous launch cleared the status word and the sync counters
extern "C" int dpg_chol_solve_gated(void* h, const double* hb, const int32_t* gate, int prezeroed, double* X,
                                    double* max_out, void* stream) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    if (!dpg_chol_gated_ok(h)) return DPG_ERR_STATE;
    c->fac_valid = false;   // (a Gauss-Newton loop's refactorizations are not tracked)
    c->has_factor = true;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (!prezeroed && (hipMemsetAsync(c->status.p, 0, sizeof(int32_t), st) != hipSuccess ||
                       hipMemsetAsync(c->sync.p, 0, c->plan.sync_bytes, st) != hipSuccess))
        return DPG_ERR_HIP;
    const bool inv = c->plan.n_inv_tasks > 0;
    if (inv) {   // this iteration's solves come after the previous iteration's inverse
        if (!c->aux.s) {
            if (hipStreamCreateWithFlags(&c->aux.s, hipStreamNonBlocking) != hipSuccess ||
                c->ev_fac.ensure(hipEventDisableTiming) || c->ev_inv[0].ensure(hipEventDisableTiming) ||
                c->ev_inv[1].ensure(hipEventDisableTiming) || hipEventRecord(c->ev_inv[0].e, c->aux.s) != hipSuccess ||
                hipEventRecord(c->ev_inv[1].e, c->aux.s) != hipSuccess)
                return DPG_ERR_HIP;
        }
        if (hipStreamWaitEvent(st, c->ev_inv[c->inv_par ^ 1].e, 0) != hipSuccess) return DPG_ERR_HIP;
    }
    launch_factor(c, st, hb, gate, nullptr);
    if (inv) {   // L11^-1 of a refactoring iteration beside its backward solve (which does not use it)
        if (hipEventRecord(c->ev_fac.e, st) != hipSuccess || hipStreamWaitEvent(c->aux.s, c->ev_fac.e, 0) != hipSuccess)
            return DPG_ERR_HIP;
        launch_inv(c, c->aux.s, gate);
        if (hipEventRecord(c->ev_inv[c->inv_par].e, c->aux.s) != hipSuccess) return DPG_ERR_HIP;
        c->inv_par ^= 1;
    }
    launch_forward(c, st, hb, nullptr, gate, c->linv.p);
    launch_backward(c, st, nullptr, gate, X, max_out, c->linv.p);
    return hipGetLastError() == hipSuccess ? DPG_OK : DPG_ERR_HIP;
}

// a Gauss-Newton graph's solver keeps L11^-1 for its chord steps (the incremental graph refactors
// every update and does not)
extern "C" void dpg_chol_keep_inverse(void* h, int on) {
    if (h) reinterpret_cast<CholDev*>(h)->keep_inv = on != 0;
}

// the gated loop's control kernel rewrites the gate the inverse kernel reads: it must come after
// this iteration's inverse (normally long finished: it ran beside the backward solve and assembly)
extern "C" int dpg_chol_join_aux(void* h, void* stream) {
    CholDev* c = reinterpret_cast<CholDev*>(h);
    if (!c || !c->aux.s) return DPG_OK;
    return hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), c->ev_inv[c->inv_par ^ 1].e, 0) == hipSuccess ? DPG_OK
                                                                                                       : DPG_ERR_HIP;
}

extern "C" const int32_t* dpg_chol_pos_dev(void* h) { return reinterpret_cast<CholDev*>(h)->pos; }
extern "C" const double* dpg_chol_x_dev(void* h) { return reinterpret_cast<CholDev*>(h)->xsol.p; }
extern "C" const int32_t* dpg_chol_status_dev(void* h) { return reinterpret_cast<CholDev*>(h)->status.p; }
extern "C" void dpg_chol_stats(void* h, double out[6]) {
    const dpg_chol_sym& S = reinterpret_cast<CholDev*>(h)->sym;
    out[0] = S.ns;
    out[1] = S.n_levels;
    out[2] = S.max_front;
    out[3] = S.flops;
    out[4] = (double)S.front_off[(size_t)S.ns] * 8.0;
    out[5] = (double)S.n;
}

// ---- selected inverse: host side ----
namespace {
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
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t nb = n + n_pairs;
    if ((rc = dpg_chol_selinv(h, stream))) return rc;
    if (c->sel_out.reserve_amortised((size_t)(9 * nb))) return DPG_ERR_HIP;
    if ((rc = dpg_chol_selinv_gather(h, nodes, n, pairs, n_pairs, c->sel_out.p, stream))) return rc;
    std::vector<double> tmp((size_t)(9 * nb));
    int32_t status = 0;
    if (hipMemcpyAsync(&status, c->status.p, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        (nb > 0 && hipMemcpyAsync(tmp.data(), c->sel_out.p, sizeof(double) * 9 * (size_t)nb, hipMemcpyDeviceToHost, st) !=
                       hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        return DPG_ERR_HIP;
    if (status != 0) return DPG_ERR_NUMERIC;
    for (double v : tmp)
        if (!(v == v)) return DPG_ERR_NUMERIC;
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
    int32_t status = 0;
    if (hipMemcpyAsync(&status, c->status.p, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(tmp.data(), c->jt_out.p, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return DPG_ERR_HIP;
    if (status != 0) return DPG_ERR_NUMERIC;
    for (double v : tmp)
        if (!(v == v)) return DPG_ERR_NUMERIC;
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

#ifdef DPG_CHOL_TIMING
extern "C" int dpg_chol_prof_dump(unsigned long long* out, int n, unsigned long long* span) {
    if (hipMemcpyFromSymbol(span, HIP_SYMBOL(g_span), sizeof(unsigned long long) * kProfL * kProfW * 2) != hipSuccess) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), sizeof(unsigned long long) * (size_t)n) == hipSuccess ? 0 : -1;
}
extern "C" int dpg_chol_steps_dump(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_steps), sizeof(unsigned long long) * 16 * 8 * (size_t)n) == hipSuccess ? 0 : -1;
}
extern "C" int dpg_chol_panel_dump(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_panel), sizeof(unsigned long long) * 16 * 8 * (size_t)n) == hipSuccess ? 0 : -1;
}
extern "C" int dpg_chol_bwd_dump(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bwd), sizeof(unsigned long long) * 8 * (size_t)n) == hipSuccess ? 0 : -1;
}
extern "C" int dpg_chol_front_dump(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_front), sizeof(unsigned long long) * 8 * (size_t)n) == hipSuccess ? 0 : -1;
}
extern "C" void dpg_chol_tree(void* h, int32_t* parent, int32_t* m3, int32_t* k3) {
    const dpg_chol_sym& S = reinterpret_cast<CholDev*>(h)->sym;
    for (int32_t s = 0; s < S.ns; ++s) {
        parent[s] = S.sn_parent[(size_t)s];
        k3[s] = 3 * (S.sn_c0[(size_t)s + 1] - S.sn_c0[(size_t)s]);
        m3[s] = k3[s] + 3 * (int32_t)(S.sn_rows_ptr[(size_t)s + 1] - S.sn_rows_ptr[(size_t)s]);
    }
}
extern "C" int dpg_chol_prof_reset(void) {
    std::vector<unsigned long long> sp((size_t)kProfL * kProfW * 2, 0ull);
    std::vector<unsigned long long> z((size_t)4096 * kProfSlots, 0ull);
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z.data(), z.size() * 8) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_span), sp.data(), sp.size() * 8) == hipSuccess ? 0 : -1;
}
#endif
