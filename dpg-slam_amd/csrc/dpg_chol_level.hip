// dpg_chol_level.hip -- the level-scheduled factorization of the GPU Cholesky (opts.fused = 0, and
// any analysis with a front past the fused kernel's LDS budget): per elimination-tree level, three
// task-list kernels over all fronts of the level (dense fronts are column-major in HBM; the task
// lists are built once per sparsity pattern by the planner, dpg_chol_plan.cpp): assemble, then per
// 48-column panel step panel and update (SYRK tiles: a large front's Schur complement is spread
// over many CUs).  fp64 throughout, explicit fma in the inner products (the solver is held to a
// tolerance, not to bit-exactness; the build keeps -ffp-contract=off for the ICP kernels).
#include "dpg_chol_dev.h"

using namespace dpg_chol;

// Phase stamps: workgroup 0 of launch `pid` into slot [pid][k]; every workgroup's start and end
#define PROF_MARK(pid, k) DPG_STAMP(blockIdx.x == 0 && threadIdx.x == 0 && (pid) < 4096, g_prof[(pid) * kProfSlots + (k)])
#define PROF_BEGIN(pid) DPG_STAMP(threadIdx.x == 0 && (pid) < kProfL && blockIdx.x < kProfW, g_span[((size_t)(pid) * kProfW + blockIdx.x) * 2])
#define PROF_END(pid) DPG_STAMP(threadIdx.x == 0 && (pid) < kProfL && blockIdx.x < kProfW, g_span[((size_t)(pid) * kProfW + blockIdx.x) * 2 + 1])
#ifdef DPG_CHOL_TIMING
constexpr int kProfSlots = 40;
__device__ unsigned long long g_prof[4096 * kProfSlots];
constexpr int kProfL = 512, kProfW = 2048;
__device__ unsigned long long g_span[kProfL * kProfW * 2];   // per launch, per workgroup: start, end
extern "C" int dpg_chol_prof_dump(unsigned long long* out, int n, unsigned long long* span) {
    if (hipMemcpyFromSymbol(span, HIP_SYMBOL(g_span), sizeof(unsigned long long) * kProfL * kProfW * 2) != hipSuccess) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), sizeof(unsigned long long) * (size_t)n) == hipSuccess ? 0 : -1;
}
extern "C" int dpg_chol_prof_reset(void) {
    std::vector<unsigned long long> sp((size_t)kProfL * kProfW * 2, 0ull);
    std::vector<unsigned long long> z((size_t)4096 * kProfSlots, 0ull);
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z.data(), z.size() * 8) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_span), sp.data(), sp.size() * 8) == hipSuccess ? 0 : -1;
}
#endif

namespace {
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

}  // namespace

void dpg_chol::launch_levels(CholDev* c, hipStream_t st, const double* hb) {
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
