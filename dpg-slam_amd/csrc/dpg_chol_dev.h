// dpg_chol_dev.h -- what the GPU Cholesky's translation units share (private to dpg_chol*.hip):
// the solver object CholDev, the layout of the sync words, the device primitives more than one
// stage uses, and one launch helper per solver kernel, defined in its kernel's file (the level
// path in dpg_chol_level.hip, the fused one in dpg_chol_factor.hip, solves and inverses in
// dpg_chol_solve.hip; dpg_chol_sel.hip launches its own; dpg_chol.hip is the driver).
#ifndef DPG_CHOL_DEV_H
#define DPG_CHOL_DEV_H

#include <hip/hip_runtime.h>

#include "dpg_chol_plan.h"
#include "dpg_ctx.h"

namespace dpg_chol {

// a requested 3x3 block of the Sigma buffer: its (0, 0) element and leading dimension (chol_selinv_pick)
struct SelPick { int64_t off; int32_t ld, pad; };

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
    DevBuf<int32_t> sync;              // plan.sync_bytes of counters and flags, zeroed per solve (sync words, below)
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
    // fronts, y and the pending updates of that factorization (identities to compare with, not owned)
    double *fac_ptr = nullptr, *fac_ysol = nullptr, *fac_acc = nullptr;
    dpg_chol_sym fac_sym;
    std::vector<int32_t> fac_G;   // (the current analysis's: plan.cur_G)
    PartialPick pick;             // the last pick: keep flags and runs (dpg_chol_plan_partial)
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

// The sync words of one solve (plan.sync_bytes, zeroed before the factorization, or before the
// forward solve where it runs alone), ns = the number of fronts:
//   [0]                    ticket of the factorization / the forward solve
//   [1, 1 + ns)            children-done counters of the same
//   [1 + ns, 1 + 2 ns)     panel flags of the large fronts
//   [1 + 2 ns]             ticket of the backward solve
//   [2 + 2 ns, 2 + 3 ns)   its done flags
//   [2 + 3 ns, ..)         pivot-tile hand-off flags, one per large-front tile
// Each kernel takes the base of its part: ticket first, then its per-front words (chol_factor_dag
// the whole array, which it cuts by ns itself).  On the host only these two know the offsets.
inline int32_t* sync_forward(CholDev* c) { return c->sync.p; }   // the factorization's too
inline int32_t* sync_backward(CholDev* c) { return c->sync.p + 1 + 2 * c->sym.ns; }

// ---- one launch site per solver kernel, in the kernel's file ----
// gate: the pipelined loop's (gate_off); keep: the partial refactorization's per-front flags; di /
// li: inverted diagonal blocks / L11^-1 for the solves' diagonal part; X, max_out: the backward
// solve retracts the poses as it goes.
void launch_levels(CholDev* c, hipStream_t st, const double* hb);
// fused factorization + forward solve of hb's system (its right-hand side follows its blocks)
void launch_factor(CholDev* c, hipStream_t st, const double* hb, const int32_t* gate, const uint8_t* keep);
// the partial path's kept fronts through c->scratch: nruns gather runs, then as many scatter runs
void launch_copy_runs(CholDev* c, hipStream_t st, const int64_t* gather, const int64_t* scatter, int64_t nruns, int64_t max_run);
void launch_forward(CholDev* c, hipStream_t st, const double* hb, const double* di, const int32_t* gate, const double* li);
void launch_backward(CholDev* c, hipStream_t st, const double* di, const int32_t* gate, double* X, double* max_out, const double* li);
// the solves' inverted diagonal blocks from the fronts just factored (opts.solve_dinv); returns the solves' `di`
const double* launch_inv_diag(CholDev* c, hipStream_t st);
// L11^-1 of the large fronts from the fronts just factored (gate: refactoring iterations only)
void launch_inv(CholDev* c, hipStream_t st, const int32_t* gate);

// Stamps of the timing builds (tools/chol_bench_t): wall_clock64() (100 MHz) into `slot` where
// `cond`; each file defines its stamp arrays, the macros over them and their dump functions.
#ifdef DPG_CHOL_TIMING
#define DPG_STAMP(cond, slot) do { if (cond) (slot) = wall_clock64(); } while (0)
#else
#define DPG_STAMP(cond, slot) do { } while (0)
#endif

// ---- device primitives of more than one stage ----
// Hand-off between workgroups (cdna_hip_programming.md Guideline 16): the payload is written with
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

// Workgroups claim fronts through an atomic ticket in topological order, so a workgroup only ever
// waits on fronts already claimed by running workgroups.
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

// v of lane l (wave-uniform l) to every lane
__device__ __forceinline__ double rdlane(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
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

}  // namespace dpg_chol

#endif
