// dpg_chol_solve.hip -- the triangular solves of the GPU Cholesky, ONE launch each with the fronts
// as a dependency DAG (forward L y = -g: leaves first; backward L^T x = y: root first; claims and
// hand-offs as dpg_chol_dev.h describes), and the inverses their diagonal part can apply instead of
// substituting (chol_inv_l11, chol_inv_diag: after a factorization).
#include "dpg_chol_dev.h"

using namespace dpg_chol;

// per diagonal block of the backward solve: [front][8 + block][0 start, 1 loaded, 2 chain, 3 column dots]
#define ST_MARK(s, p, k) DPG_STAMP(threadIdx.x == 0 && (s) < 16384 && (p) < 16 && (k) < 8, g_steps[((s) * 16 + (p)) * 8 + (k)])
// per front of the backward solve: [front][0 claim, 1 parent ready, 2 z updated, 3 solved, 4 done]
#define BW_MARK(s, k) DPG_STAMP(threadIdx.x == 0 && (s) < 16384, g_bwd[(s) * 8 + (k)])
#ifdef DPG_CHOL_TIMING
__device__ unsigned long long g_steps[16384 * 16 * 8], g_bwd[16384 * 8];
extern "C" int dpg_chol_steps_dump(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_steps), sizeof(unsigned long long) * 16 * 8 * (size_t)n) == hipSuccess ? 0 : -1;
}
extern "C" int dpg_chol_bwd_dump(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bwd), sizeof(unsigned long long) * 8 * (size_t)n) == hipSuccess ? 0 : -1;
}
#endif

namespace {
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
            const double x = rdlane(v, own);
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

// ---- the solves' diagonal blocks by substitution ----
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

}  // namespace

void dpg_chol::launch_forward(CholDev* c, hipStream_t st, const double* hb, const double* di, const int32_t* gate,
                              const double* li) {
    const CholPlan& P = c->plan;
    hipLaunchKernelGGL(chol_forward_dag, dim3(c->sym.ns), dim3(kT), P.lds_solve_max, st, c->order_fwd, sync_forward(c), c->status.p,
                       c->sns, c->child_list, c->relmap, c->fronts.p, hb + 9 * P.nnzb_upper, c->perm, c->ysol.p, c->acc.p,
                       P.solve_stage, di, gate, li);
}

void dpg_chol::launch_backward(CholDev* c, hipStream_t st, const double* di, const int32_t* gate, double* X, double* max_out,
                               const double* li) {
    const CholPlan& P = c->plan;
    hipLaunchKernelGGL(chol_backward_dag, dim3(c->sym.ns), dim3(kT), P.lds_solve_max, st, c->order_bwd, sync_backward(c),
                       c->status.p, c->sns, c->rows, c->segs, c->fronts.p, c->ysol.p, c->xsol.p, P.solve_stage, P.solve_maxseg, di, gate,
                       X ? c->perm : nullptr, X, max_out, li);
}

const double* dpg_chol::launch_inv_diag(CholDev* c, hipStream_t st) {
    const CholPlan& P = c->plan;
    if (P.use_dinv && P.n_dblocks > 0)
        hipLaunchKernelGGL(chol_inv_diag, dim3((unsigned)P.n_dblocks), dim3(64), 0, st, c->dblocks, c->sns, c->fronts.p, c->dinv.p);
    return P.use_dinv ? c->dinv.p : nullptr;
}

void dpg_chol::launch_inv(CholDev* c, hipStream_t st, const int32_t* gate) {
    const CholPlan& P = c->plan;
    if (P.n_inv_tasks > 0)
        hipLaunchKernelGGL(chol_inv_l11, dim3((unsigned)P.n_inv_tasks), dim3(kInvThreads), P.lds_inv, st, c->inv_tasks, c->sns,
                           c->fronts.p, c->linv.p, gate);
}
