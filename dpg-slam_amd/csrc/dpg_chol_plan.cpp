// dpg_chol_plan.cpp -- host planner of the GPU Cholesky (plain C++, no device call): from a symbolic
// analysis (dpg_chol_sym.cpp), the solver options and the graph's pairs to a CholPlan
// (dpg_chol_plan.h) -- the index tables the kernels of dpg_chol*.hip follow WITHOUT bounds checks
// and the launch parameters their driver reads.  One stage per function, in the order
// dpg_chol_plan_build runs them; then the pick of the partial refactorization and the joint marginals' plan.  -DDPG_PLAN_VERIFY checks the fast constructions against
// straightforward ones (tests/test_inc.py), -DDPG_PLAN_TIMING accumulates the stages' times
// (tools/incsym_bench.cpp).
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

#include "../../include/dpg_slam_c.h"
#include "dpg_chol_plan.h"

namespace dpg_chol {
namespace {

double wall_ms() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

#ifdef DPG_PLAN_TIMING
double g_plan_t[8];
#define PLAN_T(k) g_plan_t[k] += wall_ms()
#else
#define PLAN_T(k) do { } while (0)
#endif

// A child's update rows j = 0 .. 3r-1 land in parent front row 3 rm[j / 3] + j % 3, increasing in
// j: the first j landing at or after parent row c.
inline int32_t first_at_or_after(const int32_t* rm, int32_t r, int32_t c) {
    int32_t lo = 0, hi = 3 * r;
    while (lo < hi) {
        const int32_t mid = (lo + hi) / 2;
        if (3 * rm[mid / 3] + mid % 3 < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

inline int32_t rows3(const SnDev& d) { return 3 * (d.k + d.r); }

// H's upper blocks bucketed by column position, each bucket in ascending row order (pos / perm:
// the ordering -- the symbolic analysis's, or the incremental state's it will copy)
void plan_blocks(CholPlan& P, int64_t n, const int32_t* pos, const int32_t* perm, const int32_t* pair_lo,
                 const int32_t* pair_hi, int64_t n_pairs) {
    std::vector<int64_t>& colptr = P.colptr;
    colptr.assign((size_t)n + 1, 0);
    for (int64_t p = 0; p < n; ++p) colptr[(size_t)p + 1] = 1;   // the diagonal block
    for (int64_t q = 0; q < n_pairs; ++q)
        colptr[(size_t)std::min(pos[(size_t)pair_lo[q]], pos[(size_t)pair_hi[q]]) + 1]++;
    for (int64_t p = 0; p < n; ++p) colptr[(size_t)p + 1] += colptr[(size_t)p];
    std::vector<CholPlan::Blk>& ent = P.ent;
    ent.resize((size_t)colptr[(size_t)n]);
    // two counting sorts: the blocks by row (the pairs' later position; the diagonal block is its
    // column's first row), then stably into their column buckets -- each bucket comes out in
    // ascending row order without a per-bucket sort
    std::vector<int64_t>& rptr = P.om_cur;
    rptr.assign((size_t)n + 1, 0);
    for (int64_t p = 0; p < n; ++p) rptr[(size_t)p + 1] = 1;
    for (int64_t q = 0; q < n_pairs; ++q)
        rptr[(size_t)std::max(pos[(size_t)pair_lo[q]], pos[(size_t)pair_hi[q]]) + 1]++;
    for (int64_t p = 0; p < n; ++p) rptr[(size_t)p + 1] += rptr[(size_t)p];
    std::vector<CholPlan::Blk4>& byrow = P.byrow;
    byrow.resize(ent.size());
    for (int64_t p = 0; p < n; ++p) byrow[(size_t)rptr[(size_t)p]++] = CholPlan::Blk4{(int32_t)p, (int32_t)p, perm[(size_t)p], 0};
    for (int64_t q = 0; q < n_pairs; ++q) {
        const int32_t plo = pos[(size_t)pair_lo[q]], phi = pos[(size_t)pair_hi[q]];
        // front wants A(later, earlier) = H(later_node, earlier_node); hb holds H(lo, hi)
        const int32_t r = std::max(plo, phi);
        byrow[(size_t)rptr[(size_t)r]++] = CholPlan::Blk4{r, std::min(plo, phi), (int32_t)(n + q), plo > phi ? 0 : 1};
    }
    rptr.assign(colptr.begin(), colptr.end() - 1);   // column cursors
    for (const CholPlan::Blk4& b : byrow) ent[(size_t)rptr[(size_t)b.col]++] = CholPlan::Blk{b.row, b.u, b.tr};
    P.blocks_n = n;
    P.blocks_np = n_pairs;
}

// stage 1: the H-block buckets -- the prebuilt ones when they are this graph's, else built here
void block_buckets(const dpg_chol_sym& S, CholPlan& P, int64_t n, const int32_t* pair_lo, const int32_t* pair_hi,
                   int64_t n_pairs) {
    const bool pre = P.blocks_ready && P.blocks_n == n && P.blocks_np == n_pairs;
    P.blocks_ready = false;
#ifdef DPG_PLAN_VERIFY
    if (pre) {   // the prebuilt buckets must equal this plan's own
        const std::vector<int64_t> cp0 = P.colptr;
        const std::vector<CholPlan::Blk> e0 = P.ent;
        plan_blocks(P, n, S.pos.data(), S.perm.data(), pair_lo, pair_hi, n_pairs);
        bool same = cp0 == P.colptr && e0.size() == P.ent.size();
        for (size_t k = 0; same && k < e0.size(); ++k)
            same = e0[k].row == P.ent[k].row && e0[k].u == P.ent[k].u && e0[k].tr == P.ent[k].tr;
        if (!same) { fprintf(stderr, "DPG_PLAN_VERIFY: prebuilt H-block buckets differ\n"); abort(); }
    }
#endif
    if (!pre) plan_blocks(P, n, S.pos.data(), S.perm.data(), pair_lo, pair_hi, n_pairs);
}

// stage 2, omap: every upper block of H -> (front, local block row, local block col, transpose),
// grouped by front, each front's entries by (column, row): the fronts are walked column by column
// over the buckets
int block_map(const dpg_chol_sym& S, CholPlan& P, int64_t n) {
    const std::vector<int64_t>& colptr = P.colptr;
    const std::vector<CholPlan::Blk>& ent = P.ent;
    std::vector<int64_t>& om_ptr = P.om_ptr;
    om_ptr.assign((size_t)S.ns + 1, 0);
    std::vector<OEnt>& omap = P.omap;
    omap.resize(ent.size());
    std::vector<int32_t>& lidx = P.lidx;
    std::vector<int32_t>& lst = P.lstamp;
    lidx.resize((size_t)n);
    lst.assign((size_t)n, -1);
    size_t o = 0;
    for (int32_t s = 0; s < S.ns; ++s) {
        const int32_t c0 = S.sn_c0[(size_t)s], c1 = S.sn_c0[(size_t)s + 1], k = c1 - c0;
        for (int64_t t = S.sn_rows_ptr[(size_t)s]; t < S.sn_rows_ptr[(size_t)s + 1]; ++t) {
            lidx[(size_t)S.sn_rows[(size_t)t]] = k + (int32_t)(t - S.sn_rows_ptr[(size_t)s]);
            lst[(size_t)S.sn_rows[(size_t)t]] = s;
        }
        om_ptr[(size_t)s] = (int64_t)o;
        for (int32_t cpos = c0; cpos < c1; ++cpos)
            for (int64_t e = colptr[(size_t)cpos]; e < colptr[(size_t)cpos + 1]; ++e) {
                const CholPlan::Blk& b = ent[(size_t)e];
                int32_t a;
                if (b.row < c1) a = b.row - c0;
                else if (lst[(size_t)b.row] == s) a = lidx[(size_t)b.row];
                else return DPG_ERR_NUMERIC;   // the block is outside its front: bad analysis
                omap[o++] = OEnt{b.u, (int16_t)a, (int16_t)(cpos - c0), b.tr, 0};
            }
    }
    om_ptr[(size_t)S.ns] = (int64_t)o;
    return DPG_OK;
}

// stage 3: the front records, their team sizes and `need` (the children's team sizes, summed)
void front_records(const dpg_chol_sym& S, CholPlan& P, bool track) {
    std::vector<SnDev>& sns = P.sns;
    sns.resize((size_t)S.ns);
    P.acc_total = 0;
    for (int32_t s = 0; s < S.ns; ++s) {
        SnDev& d = sns[(size_t)s];
        d.c0 = S.sn_c0[(size_t)s];
        d.k = S.sn_c0[(size_t)s + 1] - d.c0;
        d.r = (int32_t)(S.sn_rows_ptr[(size_t)s + 1] - S.sn_rows_ptr[(size_t)s]);
        d.nchild = (int32_t)(S.child_ptr[(size_t)s + 1] - S.child_ptr[(size_t)s]);
        d.front_off = S.front_off[(size_t)s];
        d.rows_off = S.sn_rows_ptr[(size_t)s];
        d.child_off = S.child_ptr[(size_t)s];
        d.omap_off = P.om_ptr[(size_t)s];
        d.omap_n = (int32_t)(P.om_ptr[(size_t)s + 1] - P.om_ptr[(size_t)s]);
        d.acc_off = P.acc_total;
        d.parent = S.sn_parent[(size_t)s];
        d.G = front_team_size(rows3(d), 3 * d.k, d.nchild);
        d.need = 0;
        P.acc_total += 3 * d.r;
    }
    for (int32_t s = 0; s < S.ns; ++s)
        if (sns[(size_t)s].parent >= 0) sns[(size_t)sns[(size_t)s].parent].need += sns[(size_t)s].G;
    if (track) {
        P.cur_G.resize((size_t)S.ns);
        for (int32_t s = 0; s < S.ns; ++s) P.cur_G[(size_t)s] = sns[(size_t)s].G;
    }
}

// stage 4: L11^-1 of the fronts with at least solve_inv_cols pivot columns (and at most 64 kInvMaxQ = 192)
void inverse_tasks(const dpg_chol_sym& S, const dpg_chol_opts& o, CholPlan& P) {
    P.inv_t.clear();
    P.linv_total = 0;
    P.lds_inv = 0;
    for (int32_t s = 0; s < S.ns; ++s) {
        SnDev& d = P.sns[(size_t)s];
        const int32_t k3 = 3 * d.k;
        d.inv = -1;
        if (o.solve_inv_cols <= 0 || k3 < o.solve_inv_cols || k3 > 64 * kInvMaxQ ||
            P.linv_total + (int64_t)k3 * k3 > INT32_MAX)
            continue;
        d.inv = (int32_t)P.linv_total;
        P.linv_total += (int64_t)k3 * k3;
        for (int32_t j0 = 0; j0 < k3; j0 += kInvCols) P.inv_t.push_back(Task2{s, j0});
    }
    P.n_inv_tasks = (int64_t)P.inv_t.size();
}

// stage 5: each front's rows as segments by owning supernode (backward solve)
void solve_segments(const dpg_chol_sym& S, CholPlan& P) {
    std::vector<SolveSeg>& segs = P.segs;
    segs.clear();
    for (int32_t s = 0; s < S.ns; ++s) {
        SnDev& d = P.sns[(size_t)s];
        d.seg_off = (int32_t)segs.size();
        const int32_t* rw = S.sn_rows.data() + d.rows_off;
        for (int32_t t = 0; t < d.r;) {
            const int32_t a = S.sn_of[(size_t)rw[t]];
            int32_t t1 = t + 1;
            while (t1 < d.r && S.sn_of[(size_t)rw[t1]] == a) ++t1;
            segs.push_back(SolveSeg{a, t, t1, 0});
            t = t1;
        }
        d.seg_n = (int32_t)segs.size() - d.seg_off;
    }
}

// the omap range of front d whose block column meets the scalar columns [c0, c1)
inline void omap_range(const CholPlan& P, const SnDev& d, int32_t c0, int32_t c1, int32_t& om_b, int32_t& om_e) {
    const OEnt* ob = P.omap.data() + d.omap_off;
    om_b = (int32_t)d.omap_off + (int32_t)(std::lower_bound(ob, ob + d.omap_n, c0 / 3,
               [](const OEnt& o, int32_t v) { return o.b < v; }) - ob);
    om_e = (int32_t)d.omap_off + (int32_t)(std::upper_bound(ob, ob + d.omap_n, (c1 - 1) / 3,
               [](int32_t v, const OEnt& o) { return v < o.b; }) - ob);
}

// the tile boundaries of a large front: [0, k3) in kFNB steps, then [k3, m3) in kFNB steps
void tile_cuts(std::vector<int32_t>& cuts, int32_t k3, int32_t m3) {
    cuts.clear();
    for (int32_t c = 0; c < k3; c += kFNB) cuts.push_back(c);
    for (int32_t c = k3; c < m3; c += kFNB) cuts.push_back(c);
    cuts.push_back(m3);
}

// one large front: per tile, the H blocks (omap range) and the children's column ranges
void front_tiles(const dpg_chol_sym& S, CholPlan& P, int32_t s) {
    const std::vector<SnDev>& sns = P.sns;
    const SnDev& d = sns[(size_t)s];
    std::vector<FChild>& fchild = P.fchild;
    const int32_t k3 = 3 * d.k, m3 = rows3(d);
    std::vector<int32_t>& cuts = P.cuts;
    tile_cuts(cuts, k3, m3);
    // the children's column ranges per tile, tile-major and child order within a tile: each
    // child visits only the tiles its rows reach (its rows map to increasing front rows, so
    // the tiles' boundaries fall at increasing j), counted, then placed
    const int32_t nt = (int32_t)cuts.size() - 1;
    std::vector<int32_t>& tcnt = P.tcnt;
    tcnt.assign((size_t)nt + 1, 0);
    const int64_t ch0 = S.child_ptr[(size_t)s], ch1 = S.child_ptr[(size_t)s + 1];
    // the tile holding front row c
    const int32_t nt_k = (k3 + kFNB - 1) / kFNB;
    auto tile_of = [&](int32_t c) { return c < k3 ? c / kFNB : nt_k + (c - k3) / kFNB; };
    for (int64_t ci = ch0; ci < ch1; ++ci) {
        const SnDev& cd = sns[(size_t)S.child_list[(size_t)ci]];
        if (cd.r == 0) continue;
        const int32_t* rm = S.relmap.data() + cd.rows_off;
        const int32_t ta = tile_of(3 * rm[0]), tb = tile_of(3 * rm[cd.r - 1] + 2);
        for (int32_t t = ta; t <= tb; ++t) tcnt[(size_t)t + 1]++;   // an upper bound: empty ranges drop below
    }
    const size_t base = fchild.size();
    for (int32_t t = 0; t < nt; ++t) tcnt[(size_t)t + 1] += tcnt[(size_t)t];
    fchild.resize(base + (size_t)tcnt[(size_t)nt]);
    std::vector<int32_t>& tfill = P.tfill;
    tfill.assign(tcnt.begin(), tcnt.end() - 1);
    std::vector<char>& used = P.tused;
    used.assign(fchild.size() - base, 0);
    for (int64_t ci = ch0; ci < ch1; ++ci) {
        const SnDev& cd = sns[(size_t)S.child_list[(size_t)ci]];
        if (cd.r == 0) continue;
        const int32_t* rm = S.relmap.data() + cd.rows_off;
        const int32_t ta = tile_of(3 * rm[0]), tb = tile_of(3 * rm[cd.r - 1] + 2);
        int32_t ja = first_at_or_after(rm, cd.r, cuts[(size_t)ta]);
        for (int32_t t = ta; t <= tb; ++t) {
            const int32_t jb = first_at_or_after(rm, cd.r, cuts[(size_t)t + 1]);
            const size_t at = (size_t)tfill[(size_t)t]++;
            if (jb > ja) {
                fchild[base + at] = FChild{ja, jb, cd.k, cd.r, cd.front_off, cd.rows_off};
                used[at] = 1;
            }
            ja = jb;
        }
    }
    // compact (a child whose rows skip a whole tile left an unused slot there)
    size_t w = base;
    for (int32_t t = 0; t < nt; ++t) {
        FTask ft{0, 0, (int32_t)w, 0};
        omap_range(P, d, cuts[(size_t)t], cuts[(size_t)t + 1], ft.om_b, ft.om_e);
        for (int32_t a = tcnt[(size_t)t]; a < tcnt[(size_t)t + 1]; ++a)
            if (used[(size_t)a]) fchild[w++] = fchild[base + (size_t)a];
        ft.ch_cnt = (int32_t)w - ft.ch_off;
        P.ftasks.push_back(ft);
    }
    fchild.resize(w);
}

// stage 6: the tile tasks of every large front
void large_front_tiles(const dpg_chol_sym& S, CholPlan& P) {
    P.ftasks.clear();
    P.fchild.clear();
    for (int32_t s = 0; s < S.ns; ++s) {
        SnDev& d = P.sns[(size_t)s];
        d.ftask = (int32_t)P.ftasks.size();
        if (!front_is_small(rows3(d), d.nchild)) front_tiles(S, P, s);
    }
}

// stage 7, fused tickets (front * 64 + team member) in critical-path order: a front's priority is
// its estimated time plus its parent's priority (the longest remaining path to the root), so
// sorting by descending priority is topological (children first) and starts the long chains
// before the bulk of the leaves
void ticket_order(const dpg_chol_sym& S, CholPlan& P) {
    const std::vector<SnDev>& sns = P.sns;
    std::vector<double>& prio = P.prio;
    prio.assign((size_t)S.ns, 0.0);
    for (int32_t s = S.ns - 1; s >= 0; --s) {
        const SnDev& d = sns[(size_t)s];
        prio[(size_t)s] = front_est_us(rows3(d), 3 * d.k, d.nchild) + (d.parent >= 0 ? prio[(size_t)d.parent] : 0.0);
    }
    // (descending priority, ties in level-list order)
    std::vector<std::pair<double, int32_t>>& key = P.key;
    key.resize((size_t)S.ns);
    for (int32_t i = 0; i < S.ns; ++i) key[(size_t)i] = {-prio[(size_t)S.level_list[(size_t)i]], i};
    std::sort(key.begin(), key.end());
    std::vector<int32_t>& fo = P.fo;
    fo.resize((size_t)S.ns);
    for (int32_t i = 0; i < S.ns; ++i) fo[(size_t)i] = S.level_list[(size_t)key[(size_t)i].second];
    std::vector<int32_t>& order_fac = P.order_fac;
    order_fac.clear();
    for (int32_t s : fo)
        for (int32_t m = 0; m < sns[(size_t)s].G; ++m) order_fac.push_back(s * 64 + m);
    P.n_tickets = (int64_t)order_fac.size();
}

// stage 8: the LDS budgets of the fused factorization and the DAG solves, and the path choice
int lds_budgets(const dpg_chol_sym& S, const dpg_chol_opts& o, CholPlan& P) {
    const std::vector<SnDev>& sns = P.sns;
    // fused path: LDS budget of the largest front
    P.lds_fused = 0;
    for (int32_t s = 0; s < S.ns; ++s) {
        const SnDev& d = sns[(size_t)s];
        P.lds_fused = std::max(P.lds_fused, 8 * fused_lds_doubles(rows3(d), 3 * d.k, true));
    }
    // two panel buffers for the chain when every front fits, else one (the chain step goes through HBM)
    P.fused_db = P.lds_fused <= 160 * 1024;
    if (!P.fused_db) {
        P.lds_fused = 0;
        for (int32_t s = 0; s < S.ns; ++s) {
            const SnDev& d = sns[(size_t)s];
            P.lds_fused = std::max(P.lds_fused, 8 * fused_lds_doubles(rows3(d), 3 * d.k, false));
        }
    }
    P.fused = P.lds_fused <= 160 * 1024 && o.fused;
    // the solves' LDS: diagonal block D + staging region R + reciprocals + right-hand side / gathered
    // x + row positions, for the largest front.  Their VGPR budget (the 64-step chains) already holds
    // them to two workgroups per CU, so R defaults to what fills 80 KB; opts.solve_stage overrides it
    // (doubles, 0 = no staging)
    size_t lds_rest = 0;
    for (int32_t s = 0; s < S.ns; ++s) {
        const int32_t m3 = rows3(sns[(size_t)s]);
        lds_rest = std::max(lds_rest, (size_t)(kSB * kDL + kSB + m3 + 2 + m3 / 6 + 2 + 2 * kMaxSeg) * sizeof(double));
    }
    const long room = (long)(80 * 1024) - (long)lds_rest;
    const long want = o.solve_stage >= 0 ? (long)o.solve_stage : room / (long)sizeof(double);
    const long cap = ((long)(160 * 1024) - (long)lds_rest) / (long)sizeof(double);
    P.solve_stage = (int32_t)std::max<long>(0, std::min<long>(want, cap)) & ~1;
    // tests: 0 = every front takes the parent path
    P.solve_maxseg = o.solve_maxseg >= 0 ? std::min(o.solve_maxseg, kMaxSeg) : kMaxSeg;
    P.lds_solve_max = (size_t)P.solve_stage * sizeof(double) + lds_rest;
    return P.lds_solve_max > 160 * 1024 ? DPG_ERR_SIZE : DPG_OK;
}

// assembly tiles of front s, kCT columns each: the omap range and the children (with their
// contiguous column range) that land in the tile
void asm_tiles(const dpg_chol_sym& S, CholPlan& P, int32_t s) {
    const SnDev& d = P.sns[(size_t)s];
    const int32_t m3 = rows3(d);
    for (int32_t c0 = 0; c0 < m3; c0 += kCT) {
        const int32_t c1 = std::min(c0 + kCT, m3);
        AsmTask t{s, c0, 0, 0, (int32_t)P.asm_c.size(), 0};
        omap_range(P, d, c0, c1, t.om_b, t.om_e);
        for (int64_t ci = S.child_ptr[(size_t)s]; ci < S.child_ptr[(size_t)s + 1]; ++ci) {
            const int32_t ch = S.child_list[(size_t)ci];
            const SnDev& cd = P.sns[(size_t)ch];
            const int32_t ja = first_at_or_after(S.relmap.data() + cd.rows_off, cd.r, c0);
            const int32_t jb = first_at_or_after(S.relmap.data() + cd.rows_off, cd.r, c1);
            if (jb > ja) P.asm_c.push_back(AsmChild{ch, ja, jb, 0});
        }
        t.ch_cnt = (int32_t)P.asm_c.size() - t.ch_off;
        P.asm_t.push_back(t);
    }
}

// the panel + update steps of level l: step j0 takes the fronts with pivot columns past j0
int level_steps(const dpg_chol_sym& S, CholPlan& P, int32_t l, int32_t maxk3) {
    CholPlan::Level& L = P.levels[(size_t)l];
    for (int32_t j0 = 0; j0 < maxk3; j0 += kNB) {
        CholPlan::Step st{(int32_t)P.panel_t.size(), 0, 1, 0, (int32_t)P.upd_t.size(), 0};
        int32_t maxR = 0;
        for (int32_t q = S.level_ptr[(size_t)l]; q < S.level_ptr[(size_t)l + 1]; ++q) {
            const int32_t s = S.level_list[(size_t)q];
            const SnDev& d = P.sns[(size_t)s];
            const int32_t m3 = rows3(d), k3 = 3 * d.k;
            if (k3 <= j0) continue;
            P.panel_t.push_back(Task2{s, j0});
            maxR = std::max(maxR, m3 - j0);
            const int32_t base = j0 + std::min(kNB, k3 - j0), nt = (m3 - base + kUT - 1) / kUT;
            for (int32_t ti = 0; ti < nt; ++ti)
                for (int32_t tl = 0; tl <= ti; ++tl) P.upd_t.push_back(Task4{s, j0, base + kUT * ti, base + kUT * tl});
        }
        st.panel_cnt = (int32_t)P.panel_t.size() - st.panel_off;
        st.upd_cnt = (int32_t)P.upd_t.size() - st.upd_off;
        st.max_rows = maxR;
        st.rpt = maxR <= kT ? 1 : maxR <= 2 * kT ? 2 : maxR <= 4 * kT ? 4 : 0;
        if (st.rpt == 0) return DPG_ERR_SIZE;
        L.steps.push_back(st);
        P.n_launches += 1 + (st.upd_cnt > 0);
    }
    return DPG_OK;
}

// stage 9, the level-synchronous path (only when the fused one is off): per level, assembly
// tiles, then panel + update steps
int level_plan(const dpg_chol_sym& S, CholPlan& P) {
    P.level_ptr = S.level_ptr;
    P.asm_t.clear();
    P.asm_c.clear();
    P.panel_t.clear();
    P.upd_t.clear();
    P.levels.clear();
    P.n_launches = 0;
    if (P.fused) return DPG_OK;
    P.levels.assign((size_t)S.n_levels, CholPlan::Level{});
    for (int32_t l = 0; l < S.n_levels; ++l) {
        int32_t maxk3 = 0;
        CholPlan::Level& L = P.levels[(size_t)l];
        L.asm_off = (int32_t)P.asm_t.size();
        L.lds_asm = 0;
        for (int32_t q = S.level_ptr[(size_t)l]; q < S.level_ptr[(size_t)l + 1]; ++q) {
            const int32_t s = S.level_list[(size_t)q];
            const SnDev& d = P.sns[(size_t)s];
            L.lds_asm = std::max(L.lds_asm, (size_t)kCT * rows3(d) * sizeof(double));
            maxk3 = std::max(maxk3, 3 * d.k);
            asm_tiles(S, P, s);
        }
        L.asm_cnt = (int32_t)P.asm_t.size() - L.asm_off;
        P.n_launches += 1;
        const int rc = level_steps(S, P, l, maxk3);
        if (rc) return rc;
        if (L.lds_asm > 160 * 1024) return DPG_ERR_SIZE;
    }
    return DPG_OK;
}

// stage 10, the solves' orders: the forward solve runs in the factorization's critical-path order
// (children first); the backward solve by descending height -- the estimated time of the longest
// path from a front DOWN to a leaf, which exceeds every child's, so the order is topological
// (parents first) and the deepest chain is claimed first (the reverse of the forward order claimed
// the fronts near the root first, whatever hangs below them: a chain front could be claimed
// microseconds after its parent finished).  Also the sync words and the diagonal blocks.
void solve_orders(const dpg_chol_sym& S, const dpg_chol_opts& o, CholPlan& P) {
    const std::vector<SnDev>& sns = P.sns;
    std::vector<double>& hgt = P.hgt;
    hgt.assign((size_t)S.ns, 0.0);
    for (int32_t s = 0; s < S.ns; ++s) {   // children precede parents in supernode order
        const SnDev& d = sns[(size_t)s];
        hgt[(size_t)s] += 2.0 + 0.01 * (3 * (d.k + d.r)) + 0.05 * (3 * d.k);   // us, tools/chol_bench_t
        if (d.parent >= 0) hgt[(size_t)d.parent] = std::max(hgt[(size_t)d.parent], hgt[(size_t)s]);
    }
    // counting sort by height in 0.25 us buckets, descending; inside a bucket by descending
    // supernode index, so a parent (higher index, greater height) still precedes its children
    std::vector<int32_t>& cnt = P.hcnt;
    double hmax = 0.0;
    for (int32_t s = 0; s < S.ns; ++s) hmax = std::max(hmax, hgt[(size_t)s]);
    const int32_t nb = (int32_t)(hmax * 4.0) + 2;
    cnt.assign((size_t)nb + 1, 0);
    for (int32_t s = 0; s < S.ns; ++s) ++cnt[(size_t)(nb - 1 - (int32_t)(hgt[(size_t)s] * 4.0)) + 1];
    for (int32_t b = 0; b < nb; ++b) cnt[(size_t)b + 1] += cnt[(size_t)b];
    P.bwd.resize((size_t)S.ns);
    for (int32_t s = S.ns - 1; s >= 0; --s)
        P.bwd[(size_t)cnt[(size_t)(nb - 1 - (int32_t)(hgt[(size_t)s] * 4.0))]++] = s;
    // the sync words (layout: dpg_chol_dev.h): 2 tickets, 3 words per front,
    // one per large-front tile
    P.sync_bytes = ((size_t)(2 + 3 * S.ns + P.ftasks.size()) * sizeof(int32_t) + 15) & ~size_t(15);
    P.dblocks.clear();
    for (int32_t s = 0; s < S.ns; ++s)
        for (int32_t jb = 0; jb < 3 * sns[(size_t)s].k; jb += kSB) P.dblocks.push_back(Task2{s, jb});
    P.n_dblocks = (int64_t)P.dblocks.size();
    // measured (profiles/r03): the inversion launch (~55 us at config 4) costs more than the chains
    // it removes from the solves (re-solve 0.250 -> 0.241 ms), so the chains stay the default;
    // opts.solve_dinv selects the inverted blocks
    P.use_dinv = o.solve_dinv != 0;
}

#ifdef DPG_PLAN_VERIFY
// the straightforward construction of omap (binary search per block, per-front sort) must agree
void verify_block_map(const dpg_chol_sym& S, const CholPlan& P, int64_t n, const int32_t* pair_lo,
                      const int32_t* pair_hi, int64_t n_pairs) {
    std::vector<OEnt> ref;
    for (int32_t s = 0; s < S.ns; ++s) {
        const int32_t c0 = S.sn_c0[(size_t)s], k = S.sn_c0[(size_t)s + 1] - c0;
        auto li = [&](int32_t p) -> int32_t {
            if (p >= c0 && p < c0 + k) return p - c0;
            const int32_t* b = S.sn_rows.data() + S.sn_rows_ptr[(size_t)s];
            const int32_t* e = S.sn_rows.data() + S.sn_rows_ptr[(size_t)s + 1];
            const int32_t* it = std::lower_bound(b, e, p);
            return (it == e || *it != p) ? -1 : k + (int32_t)(it - b);
        };
        const size_t r0 = ref.size();
        for (int64_t v = 0; v < n; ++v)
            if (S.sn_of[(size_t)S.pos[(size_t)v]] == s) {
                const int32_t l = li(S.pos[(size_t)v]);
                ref.push_back(OEnt{(int32_t)v, (int16_t)l, (int16_t)l, 0, 0});
            }
        for (int64_t q = 0; q < n_pairs; ++q) {
            const int32_t plo = S.pos[(size_t)pair_lo[q]], phi = S.pos[(size_t)pair_hi[q]];
            if (S.sn_of[(size_t)std::min(plo, phi)] != s) continue;
            ref.push_back(OEnt{(int32_t)(n + q), (int16_t)li(std::max(plo, phi)), (int16_t)li(std::min(plo, phi)),
                               plo > phi ? 0 : 1, 0});
        }
        std::sort(ref.begin() + r0, ref.end(), [](const OEnt& x, const OEnt& y) { return x.b != y.b ? x.b < y.b : x.a < y.a; });
        if ((int64_t)r0 != P.om_ptr[(size_t)s]) { fprintf(stderr, "omap ptr mismatch at front %d\n", s); abort(); }
    }
    for (size_t i = 0; i < ref.size(); ++i)
        if (ref[i].u != P.omap[i].u || ref[i].a != P.omap[i].a || ref[i].b != P.omap[i].b || ref[i].tr != P.omap[i].tr) {
            fprintf(stderr, "omap mismatch at %zu\n", i);
            abort();
        }
}

// the child column ranges by a linear scan must agree
void verify_child_ranges(const dpg_chol_sym& S, const CholPlan& P) {
    const std::vector<FChild>& fchild = P.fchild;
    size_t fi = 0;
    for (int32_t s = 0; s < S.ns; ++s) {
        const SnDev& d = P.sns[(size_t)s];
        if (front_is_small(rows3(d), d.nchild)) continue;
        std::vector<int32_t> cu;
        tile_cuts(cu, 3 * d.k, rows3(d));
        for (size_t t = 0; t + 1 < cu.size(); ++t)
            for (int64_t ci = S.child_ptr[(size_t)s]; ci < S.child_ptr[(size_t)s + 1]; ++ci) {
                const SnDev& cd = P.sns[(size_t)S.child_list[(size_t)ci]];
                const int32_t* rm = S.relmap.data() + cd.rows_off;
                int32_t ja = 3 * cd.r, jb = 0;
                for (int32_t j = 0; j < 3 * cd.r; ++j) {
                    const int32_t pj = 3 * rm[j / 3] + j % 3;
                    if (pj >= cu[t] && pj < cu[t + 1]) { ja = std::min(ja, j); jb = j + 1; }
                }
                if (jb > ja) {
                    if (fi >= fchild.size() || fchild[fi].ja != ja || fchild[fi].jb != jb) {
                        fprintf(stderr, "fchild mismatch at %zu\n", fi);
                        abort();
                    }
                    ++fi;
                }
            }
    }
    if (fi != fchild.size()) { fprintf(stderr, "fchild count mismatch\n"); abort(); }
}

// the front order by a stable sort must agree, and the largest priority is the critical-path
// estimate the symbolic analysis picked the order by (the same function summed in the same order)
void verify_ticket_order(const dpg_chol_sym& S, const CholPlan& P) {
    std::vector<int32_t> ref(S.level_list.begin(), S.level_list.end());
    std::stable_sort(ref.begin(), ref.end(), [&](int32_t a, int32_t b) { return P.prio[(size_t)a] > P.prio[(size_t)b]; });
    if (ref != P.fo) { fprintf(stderr, "front order mismatch\n"); abort(); }
    double top = 0.0;
    for (double p : P.prio) top = std::max(top, p);
    if (top != dpg_chol_critical_path_us(S)) { fprintf(stderr, "critical path mismatch\n"); abort(); }
}
#endif

}  // namespace

void dpg_chol_plan_prebucket(CholPlan& P, int64_t n, const int32_t* pos, const int32_t* perm, const int32_t* pair_lo,
                             const int32_t* pair_hi, int64_t n_pairs) {
    P.blocks_ready = false;
    plan_blocks(P, n, pos, perm, pair_lo, pair_hi, n_pairs);
    P.blocks_ready = true;
}

int dpg_chol_plan_build(CholPlan& P, const dpg_chol_sym& S, const dpg_chol_opts& o, bool track, int64_t n,
                        const int32_t* pair_lo, const int32_t* pair_hi, int64_t n_pairs) {
    P.n = n;
    P.nnzb_upper = n + n_pairs;
    PLAN_T(0);
    block_buckets(S, P, n, pair_lo, pair_hi, n_pairs);
    PLAN_T(1);
    int rc = block_map(S, P, n);
    if (rc) return rc;
#ifdef DPG_PLAN_VERIFY
    verify_block_map(S, P, n, pair_lo, pair_hi, n_pairs);
#endif
    PLAN_T(2);
    front_records(S, P, track);
    inverse_tasks(S, o, P);
    solve_segments(S, P);
    PLAN_T(3);
    large_front_tiles(S, P);
#ifdef DPG_PLAN_VERIFY
    verify_child_ranges(S, P);
#endif
    PLAN_T(4);
    ticket_order(S, P);
#ifdef DPG_PLAN_VERIFY
    verify_ticket_order(S, P);
#endif
    PLAN_T(5);
    if ((rc = lds_budgets(S, o, P)) != DPG_OK || (rc = level_plan(S, P)) != DPG_OK) return rc;
    PLAN_T(6);
    solve_orders(S, o, P);
    PLAN_T(7);
    return DPG_OK;
}

// ---- partial refactorization: the kept fronts and the runs that move them ----
bool dpg_chol_plan_partial(PartialPick& K, const dpg_chol_sym& S, const dpg_chol_sym& O, const std::vector<int32_t>& cur_G,
                           const std::vector<int32_t>& fac_G, const int32_t* dirty_nodes, int64_t n_dirty) {
    const int32_t ns = S.ns;
    K.keep.assign((size_t)ns, 1);
    K.old.assign((size_t)ns, -1);
    for (int64_t q = 0; q < n_dirty; ++q) {
        const int32_t v = dirty_nodes[q];
        if (v < 0 || v >= S.n) return false;
        K.keep[(size_t)S.sn_of[(size_t)S.pos[(size_t)v]]] = 0;
    }
    K.kept = 0;
    for (int32_t sn = 0; sn < ns; ++sn) {   // children before parents (a parent's first column is later)
        if (K.keep[(size_t)sn]) {
            const int32_t c0 = S.sn_c0[(size_t)sn], c1 = S.sn_c0[(size_t)sn + 1];
            bool same = c1 <= O.n;
            int32_t os = -1;
            if (same) {
                os = O.sn_of[(size_t)c0];
                same = O.sn_c0[(size_t)os] == c0 && O.sn_c0[(size_t)os + 1] == c1 && fac_G[(size_t)os] == cur_G[(size_t)sn];
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
                K.old[(size_t)sn] = os;
                ++K.kept;
            } else {
                K.keep[(size_t)sn] = 0;
            }
        }
        if (!K.keep[(size_t)sn] && S.sn_parent[(size_t)sn] >= 0) K.keep[(size_t)S.sn_parent[(size_t)sn]] = 0;
    }
    if (K.kept == 0) return false;
    // runs of kept fronts the layout moved (front s's pending updates sit at 3 sn_rows_ptr[s]: the plan's acc_off)
    std::vector<int64_t>& runs = K.runs;
    runs.clear();
    K.moved = K.max_run = 0;
    auto add_run = [&](int64_t src, int64_t dst, int64_t len, int64_t buf) {
        if (src == dst || len == 0) return;
        const size_t nr = runs.size();
        if (nr >= 4 && runs[nr - 1] == buf && runs[nr - 4] + runs[nr - 2] == src && runs[nr - 3] + runs[nr - 2] == dst) {
            runs[nr - 2] += len;
        } else {
            runs.insert(runs.end(), {src, dst, len, buf});
        }
        K.max_run = std::max(K.max_run, runs[runs.size() - 2]);
        K.moved += len;
    };
    for (int32_t sn = 0; sn < ns; ++sn)
        if (K.keep[(size_t)sn])
            add_run(O.front_off[(size_t)K.old[(size_t)sn]], S.front_off[(size_t)sn],
                    S.front_off[(size_t)sn + 1] - S.front_off[(size_t)sn], 0);
    for (int32_t sn = 0; sn < ns; ++sn)
        if (K.keep[(size_t)sn])
            add_run(3 * O.sn_rows_ptr[(size_t)K.old[(size_t)sn]], 3 * S.sn_rows_ptr[(size_t)sn],
                    3 * (S.sn_rows_ptr[(size_t)sn + 1] - S.sn_rows_ptr[(size_t)sn]), 1);
    return runs.size() / 4 <= 65535;
}

// ---- joint marginals: root paths, W slices and per-block suffixes ----
namespace {

void joint_begin(JointPlan& J, const dpg_chol_sym& S) {
    J.nodes.clear();
    J.queries.clear();
    J.path_ptr.assign(1, 0);
    J.path_sn.clear();
    J.path_len.clear();
    J.len.clear();
    J.pairs.clear();
    J.w_total = 0;
    J.slot.assign((size_t)S.n, -1);
}

// the query of node v (a new one walks sn_parent from v's front to its root)
int32_t joint_query(JointPlan& J, const dpg_chol_sym& S, int32_t v) {
    if (J.slot[(size_t)v] >= 0) return J.slot[(size_t)v];
    const int32_t q = (int32_t)J.nodes.size();
    const int32_t p = S.pos[(size_t)v];
    const int32_t s0 = S.sn_of[(size_t)p];
    int64_t len = 0;
    for (int32_t s = s0; s >= 0; s = S.sn_parent[(size_t)s]) {
        const int32_t k3 = 3 * (S.sn_c0[(size_t)s + 1] - S.sn_c0[(size_t)s]);
        J.path_sn.push_back(s);
        J.path_len.push_back(k3);
        len += k3;
    }
    J.path_ptr.push_back((int64_t)J.path_sn.size());
    J.nodes.push_back(v);
    J.queries.push_back(PathQuery{s0, 3 * (p - S.sn_c0[(size_t)s0]), J.w_total});
    J.len.push_back(len);
    J.w_total += 3 * len;
    J.slot[(size_t)v] = q;
    return q;
}

// block Sigma(u, v) to o and its transpose to ot (either may be -1).  The product is taken with
// the smaller node's slice on the left, so (u, v) and (v, u) are one computation and its mirror.
void joint_block(JointPlan& J, const dpg_chol_sym& S, int32_t u, int32_t v, int64_t o, int64_t ot) {
    if (u > v) {
        std::swap(u, v);
        std::swap(o, ot);
    }
    const int32_t qa = joint_query(J, S, u), qb = joint_query(J, S, v);
    // the common suffix of the two paths: equal fronts from the roots' end
    int64_t ea = J.path_ptr[(size_t)qa + 1], eb = J.path_ptr[(size_t)qb + 1];
    const int64_t ba = J.path_ptr[(size_t)qa], bb = J.path_ptr[(size_t)qb];
    int64_t len = 0;
    while (ea > ba && eb > bb && J.path_sn[(size_t)ea - 1] == J.path_sn[(size_t)eb - 1]) {
        len += J.path_len[(size_t)ea - 1];
        --ea;
        --eb;
    }
    PathPair t;
    t.a = J.queries[(size_t)qa].w_off + 3 * (J.len[(size_t)qa] - len);
    t.b = J.queries[(size_t)qb].w_off + 3 * (J.len[(size_t)qb] - len);
    t.o = o;
    t.ot = ot;
    t.len = (int32_t)len;
    t.pad = 0;
    J.pairs.push_back(t);
}

}  // namespace

void dpg_chol_plan_joint_pairs(JointPlan& J, const dpg_chol_sym& S, const int32_t* pairs, int64_t n) {
    joint_begin(J, S);
    J.ld = 3;
    J.out_total = 9 * n;
    for (int64_t q = 0; q < n; ++q) joint_block(J, S, pairs[2 * q], pairs[2 * q + 1], 9 * q, -1);
}

void dpg_chol_plan_joint_nodes(JointPlan& J, const dpg_chol_sym& S, const int32_t* nodes, int64_t n) {
    joint_begin(J, S);
    J.ld = (int32_t)(3 * n);
    J.out_total = 9 * n * n;
    for (int64_t p = 0; p < n; ++p)
        for (int64_t q = p; q < n; ++q)
            joint_block(J, S, nodes[p], nodes[q], 3 * p * J.ld + 3 * q, q > p ? 3 * q * J.ld + 3 * p : -1);
}

}  // namespace dpg_chol

#ifdef DPG_PLAN_TIMING
double dpg_plan_t_export[8];
#endif
int dpg_chol_plan_host(int64_t n, const int32_t* pair_lo, const int32_t* pair_hi, int64_t n_pairs,
                       const dpg_chol_sym* S, const dpg_chol_opts* opts, double* ms) {
    thread_local dpg_chol::CholPlan P;
    const dpg_chol_opts o = opts ? *opts : dpg_chol_opts();
    const double t0 = dpg_chol::wall_ms();
    const int rc = dpg_chol::dpg_chol_plan_build(P, *S, o, false, n, pair_lo, pair_hi, n_pairs);
    if (ms) *ms = dpg_chol::wall_ms() - t0;
#ifdef DPG_PLAN_TIMING
    for (int k = 0; k < 8; ++k) dpg_plan_t_export[k] = dpg_chol::g_plan_t[k];
#endif
    return rc;
}
