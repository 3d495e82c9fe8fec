// sanitize_check.cpp -- the host C / C++ code under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make -C oracle sanitize`, run by tests/test_sanitize.py in the CPU suite): the oracle
// (dpg_oracle.c, dpg_change_oracle.cpp), the host half of the C ABI (csrc/dpg_host.c), the
// synthetic workload generator (csrc/dpg_synth.c), the symbolic Cholesky analysis, full and
// incremental (csrc/dpg_chol_sym.cpp), and the GPU solver's host planner (csrc/dpg_chol_plan.cpp:
// its tables are followed by the kernels without bounds checks; its pick of the fronts a partial
// refactorization keeps, and of the runs that move them, against the pick's contract) and change
// detection's host plan (csrc/dpg_change_plan.cpp: window reuse and bit-plane bookkeeping against
// values worked out by hand), driven through a small
// end-to-end workload: scans -> clouds -> batched ICP + covariance -> factors -> Gauss-Newton ->
// symbolic analysis -> solver plans -> DPG change detection over two passes; the owning buffer
// template of the GPU layer (csrc/dpg_buf.h) over host memory; and the pose graphs' contribution
// lists (dpg_contribution_lists) against a per-block construction.  Any sanitizer report aborts
// (-fno-sanitize-recover).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <vector>

#include "../dpg-slam_amd/csrc/dpg_buf.h"
#include "../dpg-slam_amd/csrc/dpg_change_plan.h"
#include "../dpg-slam_amd/csrc/dpg_chol.h"
#include "../dpg-slam_amd/csrc/dpg_chol_plan.h"
#include "../dpg-slam_amd/csrc/dpg_internal.h"
#include "../oracle/dpg_oracle.h"

struct oracle_dpg;
extern "C" {
oracle_dpg* oracle_dpg_create(int64_t V, const int64_t* off, const float* ranges, const float* geom,
                              const dpg_change_params* p);
void oracle_dpg_destroy(oracle_dpg* o);
int oracle_dpg_append(oracle_dpg* o, int64_t n, const int64_t* off, const float* ranges, const float* geom);
int oracle_execute_dpg(oracle_dpg* o, int64_t V, int64_t cur_len, const float* est, dpg_change_stats* st);
void oracle_dpg_fetch(oracle_dpg* o, uint8_t* labels, uint8_t* sector_active, uint8_t* node_active);
int64_t oracle_active_dynamic_points(oracle_dpg* o, int64_t V, const float* est, float* out, int64_t cap,
                                     int64_t counts[4]);
}

#define REQUIRE(c)                                                         \
    do {                                                                   \
        if (!(c)) { fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

// The solver plan of one graph under each option set that selects another branch of the planner
// (the fused DAG path, the level path, L11^-1 tasks, inverted diagonal blocks), tracked and not,
// and once more from buckets prebuilt ahead of the plan.  want_team: the graph must have a front
// factored by a team, and its level plan a step with trailing-update tiles.
static int plan_graph(int64_t n, const std::vector<int32_t>& lo, const std::vector<int32_t>& hi, bool want_team) {
    using dpg_chol::CholPlan;
    const int64_t np = (int64_t)lo.size();
    dpg_chol_opts base{64, 0.3};
    dpg_chol_sym S;
    REQUIRE(dpg_chol_symbolic(n, lo.data(), hi.data(), np, &base, &S) == 0);
    dpg_chol_opts sets[4] = {base, base, base, base};
    sets[1].fused = 0;
    sets[2].solve_inv_cols = 48;
    sets[3].solve_dinv = 1;
    CholPlan P;   // one plan object reused, as the solver reuses its own between builds
    for (int k = 0; k < 4; ++k)
        for (int track = 0; track < 2; ++track) {
            REQUIRE(dpg_chol_plan_build(P, S, sets[k], track != 0, n, lo.data(), hi.data(), np) == DPG_OK);
            REQUIRE(P.fused == (k != 1) && (int64_t)P.sns.size() == S.ns && (int64_t)P.bwd.size() == S.ns);
            REQUIRE((P.n_inv_tasks > 0) == (k == 2) && P.use_dinv == (k == 3) && P.n_dblocks >= S.ns);
            REQUIRE(!track || (int64_t)P.cur_G.size() == S.ns);
            bool team = false, upd = false;
            for (const dpg_chol::SnDev& d : P.sns) team = team || d.G > 1;
            for (const CholPlan::Level& L : P.levels)
                for (const CholPlan::Step& st : L.steps) upd = upd || st.upd_cnt > 0;
            if (want_team) REQUIRE(team && !P.ftasks.empty());
            if (want_team && k == 1) REQUIRE(upd);
            REQUIRE((k == 1) == !P.levels.empty());
        }
    const std::vector<dpg_chol::OEnt> omap = P.omap;
    dpg_chol_plan_prebucket(P, n, S.pos.data(), S.perm.data(), lo.data(), hi.data(), np);
    REQUIRE(dpg_chol_plan_build(P, S, base, false, n, lo.data(), hi.data(), np) == DPG_OK);
    REQUIRE(P.omap.size() == omap.size() && memcmp(P.omap.data(), omap.data(), omap.size() * sizeof(omap[0])) == 0);
    double ms = 0;
    REQUIRE(dpg_chol_plan_host(n, lo.data(), hi.data(), np, &S, nullptr, &ms) == DPG_OK);
    return 0;
}

// One pick of the partial refactorization (dpg_chol_plan_partial) against its contract: (a) no kept
// front holds a dirty node's column or lies above a front that is not kept; (b) a kept front's old
// front has its columns, rows, children and team size; (c) the runs, applied as chol_copy_runs
// applies them (all gathers into the scratch, then all scatters), leave every kept front's values
// and pending rows at their new places and write nothing else.
static int pick_holds(const dpg_chol::PartialPick& K, const dpg_chol_sym& S, const dpg_chol_sym& O,
                      const std::vector<int32_t>& cur_G, const std::vector<int32_t>& fac_G, const std::vector<int32_t>& dirty) {
    const size_t ns = (size_t)S.ns;
    REQUIRE(K.keep.size() == ns && K.old.size() == ns && K.runs.size() % 4 == 0);
    for (int32_t v : dirty) REQUIRE(!K.keep[(size_t)S.sn_of[(size_t)S.pos[(size_t)v]]]);
    int64_t kept = 0;
    for (size_t s = 0; s < ns; ++s) {
        if (!K.keep[s]) {   // (by induction: nothing above a front that is not kept is kept)
            REQUIRE(K.old[s] == -1 && (S.sn_parent[s] < 0 || !K.keep[(size_t)S.sn_parent[s]]));
            continue;
        }
        ++kept;
        REQUIRE(K.old[s] >= 0 && K.old[s] < O.ns);
        const size_t o = (size_t)K.old[s];
        REQUIRE(S.sn_c0[s] == O.sn_c0[o] && S.sn_c0[s + 1] == O.sn_c0[o + 1] && cur_G[s] == fac_G[o]);
        const int64_t r0 = S.sn_rows_ptr[s], nr = S.sn_rows_ptr[s + 1] - r0, q0 = O.sn_rows_ptr[o];
        REQUIRE(nr == O.sn_rows_ptr[o + 1] - q0 && std::equal(S.sn_rows.begin() + r0, S.sn_rows.begin() + r0 + nr, O.sn_rows.begin() + q0));
        const int64_t a0 = S.child_ptr[s], nc = S.child_ptr[s + 1] - a0, b0 = O.child_ptr[o];
        REQUIRE(nc == O.child_ptr[o + 1] - b0);
        for (int64_t t = 0; t < nc; ++t)
            REQUIRE(S.sn_c0[(size_t)S.child_list[(size_t)(a0 + t)]] == O.sn_c0[(size_t)O.child_list[(size_t)(b0 + t)]]);
    }
    REQUIRE(kept == K.kept && kept > 0);
    // buffer 0: the fronts, buffer 1: the pending updates (front s at 3 sn_rows_ptr[s]); every old
    // double encodes (front, offset), -1 outside the old layout
    const auto enc = [](size_t front, int64_t off) { return (double)front * 4294967296.0 + (double)off; };
    const int64_t old_end[2] = {O.front_off[(size_t)O.ns], 3 * O.sn_rows_ptr[(size_t)O.ns]};
    const int64_t new_end[2] = {S.front_off[ns], 3 * S.sn_rows_ptr[ns]};
    std::vector<double> buf[2], scratch((size_t)K.moved, -2.0);
    std::vector<uint8_t> written[2];
    for (int b = 0; b < 2; ++b) {
        buf[b].assign((size_t)std::max(old_end[b], new_end[b]), -1.0);
        written[b].assign(buf[b].size(), 0);
    }
    for (size_t o = 0; o < (size_t)O.ns; ++o) {
        for (int64_t e = O.front_off[o]; e < O.front_off[o + 1]; ++e) buf[0][(size_t)e] = enc(o, e - O.front_off[o]);
        for (int64_t e = 3 * O.sn_rows_ptr[o]; e < 3 * O.sn_rows_ptr[o + 1]; ++e) buf[1][(size_t)e] = enc(o, e - 3 * O.sn_rows_ptr[o]);
    }
    int64_t off = 0, max_run = 0;
    for (size_t r = 0; r < K.runs.size(); r += 4) {   // gather {src, scratch}
        const int64_t src = K.runs[r], len = K.runs[r + 2], b = K.runs[r + 3];
        REQUIRE((b == 0 || b == 1) && len > 0 && src >= 0 && src + len <= old_end[b] && off + len <= K.moved);
        std::copy(buf[b].begin() + src, buf[b].begin() + src + len, scratch.begin() + off);
        off += len;
        max_run = std::max(max_run, len);
    }
    REQUIRE(off == K.moved && max_run == K.max_run);
    off = 0;
    for (size_t r = 0; r < K.runs.size(); r += 4) {   // scatter {scratch, dst}
        const int64_t dst = K.runs[r + 1], len = K.runs[r + 2], b = K.runs[r + 3];
        REQUIRE(dst >= 0 && dst + len <= new_end[b]);
        std::copy(scratch.begin() + off, scratch.begin() + off + len, buf[b].begin() + dst);
        std::fill(written[b].begin() + dst, written[b].begin() + dst + len, 1);
        off += len;
    }
    for (size_t s = 0; s < ns; ++s) {
        if (!K.keep[s]) continue;
        const int64_t lo[2] = {S.front_off[s], 3 * S.sn_rows_ptr[s]}, hi[2] = {S.front_off[s + 1], 3 * S.sn_rows_ptr[s + 1]};
        for (int b = 0; b < 2; ++b)
            for (int64_t e = lo[b]; e < hi[b]; ++e) {
                REQUIRE(buf[b][(size_t)e] == enc((size_t)K.old[s], e - lo[b]));
                written[b][(size_t)e] = 0;
            }
    }
    for (int b = 0; b < 2; ++b) REQUIRE(std::find(written[b].begin(), written[b].end(), 1) == written[b].end());
    return 0;
}

// The pick for a graph analysed before and after node n with edges to `nbr` is appended, through the
// incremental symbolic analysis as the incremental graph runs it (the old order is a prefix of the
// new one), then its exceptions: a dirty node out of range, every node dirty, one leaf front dirty.
static int partial_graph(int64_t n, std::vector<int32_t> lo, std::vector<int32_t> hi, const std::vector<int32_t>& nbr,
                         int64_t* kept, int64_t* moved) {
    using dpg_chol::dpg_chol_plan_partial;
    const dpg_chol_opts o{64, 0.3};
    dpg_chol_incsym I;
    dpg_chol_sym O, S;
    dpg_chol::CholPlan P;
    REQUIRE(dpg_incsym_reset(&I, n, lo.data(), hi.data(), (int64_t)lo.size(), &o) == 0 && dpg_incsym_derive(&I, &o, &O) == 0);
    REQUIRE(dpg_chol_plan_build(P, O, o, true, n, lo.data(), hi.data(), (int64_t)lo.size()) == DPG_OK);
    const std::vector<int32_t> fac_G = P.cur_G;
    dpg_incsym_append(&I, 1);
    std::vector<int32_t> dirty(1, (int32_t)n);
    for (int32_t u : nbr) {
        dpg_incsym_add_edge(&I, u, (int32_t)n);
        lo.push_back(u);
        hi.push_back((int32_t)n);
        dirty.push_back(u);
    }
    REQUIRE(dpg_incsym_derive(&I, &o, &S) == 0);
    REQUIRE(dpg_chol_plan_build(P, S, o, true, n + 1, lo.data(), hi.data(), (int64_t)lo.size()) == DPG_OK);
    REQUIRE(O.n == n && S.n == n + 1 && std::equal(O.perm.begin(), O.perm.end(), S.perm.begin()));
    REQUIRE((int64_t)fac_G.size() == O.ns && (int64_t)P.cur_G.size() == S.ns);
    dpg_chol::PartialPick K;
    REQUIRE(dpg_chol_plan_partial(K, S, O, P.cur_G, fac_G, dirty.data(), (int64_t)dirty.size()));
    REQUIRE(pick_holds(K, S, O, P.cur_G, fac_G, dirty) == 0 && K.kept < S.ns);
    *kept = K.kept;
    *moved = K.moved;
    const int32_t out[4] = {nbr[0], (int32_t)(n + 1), nbr[0], -1};
    REQUIRE(!dpg_chol_plan_partial(K, S, O, P.cur_G, fac_G, out, 2) && !dpg_chol_plan_partial(K, S, O, P.cur_G, fac_G, out + 2, 2));
    std::vector<int32_t> all((size_t)n + 1);
    for (size_t v = 0; v < all.size(); ++v) all[v] = (int32_t)v;
    REQUIRE(!dpg_chol_plan_partial(K, S, O, P.cur_G, fac_G, all.data(), (int64_t)all.size()));
    int32_t leaf = -1;   // a childless front of old columns, not the new node's
    for (int32_t s = 0; s < S.ns && leaf < 0; ++s)
        if (S.child_ptr[(size_t)s] == S.child_ptr[(size_t)s + 1] && S.sn_c0[(size_t)s + 1] <= O.n && S.sn_parent[(size_t)s] >= 0) leaf = s;
    REQUIRE(leaf >= 0);
    const std::vector<int32_t> one(1, S.perm[(size_t)S.sn_c0[(size_t)leaf]]);
    REQUIRE(dpg_chol_plan_partial(K, S, O, P.cur_G, fac_G, one.data(), 1) && K.kept > 0 && !K.keep[(size_t)leaf]);
    REQUIRE(pick_holds(K, S, O, P.cur_G, fac_G, one) == 0);
    return 0;
}

static int plan_checks() {
    std::vector<int32_t> lo, hi;
    int64_t kept[2] = {0, 0}, moved[2] = {0, 0};
    const int M = 30;   // M x M 4-neighbour mesh: separator fronts past the in-LDS limit (teams)
    for (int r = 0; r < M; ++r)
        for (int c = 0; c < M; ++c) {
            if (c + 1 < M) { lo.push_back(r * M + c); hi.push_back(r * M + c + 1); }
            if (r + 1 < M) { lo.push_back(r * M + c); hi.push_back((r + 1) * M + c); }
        }
    REQUIRE(plan_graph(M * M, lo, hi, true) == 0);
    REQUIRE(partial_graph(M * M, lo, hi, {M * M - 1, M * M - 2, M - 1}, &kept[0], &moved[0]) == 0);
    // a 700-node chain with up to three random loop closures per node (tests/test_inc.py's graph)
    lo.clear();
    hi.clear();
    uint32_t x = 5;
    auto rnd = [&x](uint32_t m) { x = x * 1664525u + 1013904223u; return (int32_t)((x >> 8) % m); };
    for (int v = 1; v < 700; ++v) {
        int32_t e[4] = {v - 1, -1, -1, -1};
        int ne = 1;
        for (int k = v > 20 ? rnd(4) : 0; k > 0; --k) {
            const int32_t u = rnd((uint32_t)(v - 10));
            if (std::find(e, e + ne, u) == e + ne) e[ne++] = u;
        }
        for (int k = 0; k < ne; ++k) { lo.push_back(e[k]); hi.push_back(v); }
    }
    REQUIRE(plan_graph(700, lo, hi, false) == 0);
    REQUIRE(partial_graph(700, lo, hi, {699, 350}, &kept[1], &moved[1]) == 0);
    printf("solver plans ok: %d x %d mesh, 700-node loop graph\n", M, M);
    REQUIRE(moved[0] + moved[1] > 0);   // (the runs were exercised)
    printf("partial pick ok: one node appended, %lld and %lld fronts kept, %lld and %lld doubles moved\n", (long long)kept[0],
           (long long)kept[1], (long long)moved[0], (long long)moved[1]);
    return 0;
}

// OwnedBuf's growth rules and ownership over malloc / free / memcpy: the policy counts allocations
// and live bytes (the size sits in a 16-byte header before each block) and can be told to fail the
// next allocation.
struct HostMem {
    typedef int stream_t;
    static int allocs, fail_next;
    static size_t live;
    static int alloc(void** p, size_t bytes) {
        if (fail_next) { fail_next = 0; return -1; }
        char* b = static_cast<char*>(malloc(bytes + 16));
        if (!b) return -1;
        memcpy(b, &bytes, sizeof(bytes));
        ++allocs;
        live += bytes;
        *p = b + 16;
        return 0;
    }
    static void free(void* p) {
        char* b = static_cast<char*>(p) - 16;
        size_t bytes;
        memcpy(&bytes, b, sizeof(bytes));
        live -= bytes;
        ::free(b);
    }
    static int copy(void* dst, const void* src, size_t bytes, int) {
        memcpy(dst, src, bytes);
        return 0;
    }
};
int HostMem::allocs = 0, HostMem::fail_next = 0;
size_t HostMem::live = 0;

static int buffer_checks() {
    typedef OwnedBuf<int32_t, HostMem> Buf;
    {   // (a) the amortised rule from empty, max(n, cap + cap / 2): 13 allocations for n = 1..100
        const size_t want[13] = {1, 2, 3, 4, 6, 9, 13, 19, 28, 42, 63, 94, 141};
        Buf b;
        int k = 0;
        for (size_t n = 1; n <= 100; ++n) {
            const int before = HostMem::allocs;
            REQUIRE(b.reserve_amortised(n) == 0 && b.p && b.cap >= n);
            if (HostMem::allocs != before) {
                REQUIRE(HostMem::allocs == before + 1 && k < 13 && b.cap == want[k]);
                ++k;
            }
            REQUIRE(HostMem::live == b.cap * sizeof(int32_t));   // released first: one buffer at any time
        }
        REQUIRE(k == 13);
        // with slack every capacity is the rule's value (from the capacity held) plus the slack: for
        // n = 1..100 that is one allocation of 1 + 4096, and past it the 1.5x step or n, plus 4096
        Buf c;
        const int a0 = HostMem::allocs;
        for (size_t n = 0; n <= 100; ++n) REQUIRE(c.reserve_amortised(n, 4096) == 0 && c.cap == 1 + 4096);
        REQUIRE(HostMem::allocs == a0 + 1);
        const size_t ask[5] = {4098, 6000, 20000, 20001, 40000};
        const size_t get[5] = {4097 + 2048 + 4096, 10241, 20000 + 4096, 24096, 40000 + 4096};   // 1.5x, -, n, -, n
        for (int q = 0; q < 5; ++q) REQUIRE(c.reserve_amortised(ask[q], 4096) == 0 && c.cap == get[q]);
        REQUIRE(HostMem::allocs == a0 + 4 && HostMem::live == (b.cap + c.cap) * sizeof(int32_t));
        // (c) a failed amortised reserve leaves the buffer empty
        HostMem::fail_next = 1;
        REQUIRE(c.reserve_amortised(100000) == -1 && c.p == nullptr && c.cap == 0);
        REQUIRE(c.reserve(0) == 0 && c.p == nullptr);   // exact form: nothing asked of an empty buffer, nothing made
        REQUIRE(c.reserve(7) == 0 && c.cap == 7 && c.reserve(5) == 0 && c.cap == 7);
    }
    REQUIRE(HostMem::live == 0);
    {   // (b) grow keeps the first min(keep, old capacity) elements; a failed grow changes nothing
        Buf b;
        REQUIRE(b.grow(0, 0, 0) == 0 && b.p == nullptr);   // (no clamp: the callers that can ask for 0 clamp)
        REQUIRE(b.grow(10, 0, 0) == 0 && b.cap == 10);
        for (int i = 0; i < 10; ++i) b.p[i] = 1000 + i;
        REQUIRE(b.grow(11, 6, 0) == 0 && b.cap == 15);    // 10 + 10 / 2
        for (int i = 0; i < 6; ++i) REQUIRE(b.p[i] == 1000 + i);
        for (int i = 6; i < 15; ++i) b.p[i] = 2000 + i;
        REQUIRE(b.grow(100, 1000, 0) == 0 && b.cap == 100);   // keep past the old capacity: all 15 kept
        for (int i = 0; i < 15; ++i) REQUIRE(b.p[i] == (i < 6 ? 1000 : 2000) + i);
        int32_t* p0 = b.p;
        HostMem::fail_next = 1;
        REQUIRE(b.grow(1000, 15, 0) == -1 && b.p == p0 && b.cap == 100);
        for (int i = 0; i < 15; ++i) REQUIRE(b.p[i] == (i < 6 ? 1000 : 2000) + i);
        REQUIRE(b.grow(100, 15, 0) == 0 && b.p == p0);        // nothing to do
        // (d) one owner per allocation through move construction, move assignment and std::swap
        const size_t live1 = HostMem::live;
        Buf m(std::move(b));
        REQUIRE(b.p == nullptr && b.cap == 0 && m.p == p0 && m.cap == 100 && HostMem::live == live1);
        Buf o;
        REQUIRE(o.reserve(3) == 0);
        int32_t* p1 = o.p;
        o = std::move(m);   // move-assignment swaps: the moved-from buffer owns the other allocation
        REQUIRE(o.p == p0 && o.cap == 100 && m.p == p1 && m.cap == 3);
        std::swap(o, m);
        REQUIRE(o.p == p1 && o.cap == 3 && m.p == p0 && m.cap == 100);
        REQUIRE(HostMem::live == (100 + 3) * sizeof(int32_t));
        m.release();
        REQUIRE(m.p == nullptr && m.cap == 0 && HostMem::live == 3 * sizeof(int32_t));
    }
    REQUIRE(HostMem::live == 0 && HostMem::fail_next == 0);
    printf("buffers ok: %d allocations, none live\n", HostMem::allocs);
    return 0;
}

// dpg_contribution_lists against a per-block construction: block u's list is, factor by factor, the
// entries whose block is u.  pairs are (lo, hi) in the caller's order; a Between's pair is looked up.
static int lists_case(int64_t n, const std::vector<dpg_factor>& F, const std::vector<int32_t>& lo,
                      const std::vector<int32_t>& hi) {
    const int64_t nf = (int64_t)F.size(), P = (int64_t)lo.size(), nu = n + P;
    std::vector<int32_t> pair((size_t)nf, -1);
    size_t n_list = 0;
    for (int64_t k = 0; k < nf; ++k) {
        n_list += F[(size_t)k].kind == DPG_FACTOR_BETWEEN ? 3 : 1;
        if (F[(size_t)k].kind != DPG_FACTOR_BETWEEN) continue;
        for (int64_t p = 0; p < P; ++p)
            if (lo[(size_t)p] == std::min(F[(size_t)k].i, F[(size_t)k].j) && hi[(size_t)p] == std::max(F[(size_t)k].i, F[(size_t)k].j))
                pair[(size_t)k] = (int32_t)p;
        REQUIRE(pair[(size_t)k] >= 0);
    }
    // exact sizes, so that a write past either array is the sanitizer's to report
    std::vector<int32_t> cptr((size_t)nu + 1, -7), clist(n_list, -7), want;
    dpg_contribution_lists(F.data(), nf, n, pair.data(), P, cptr.data(), clist.data());
    REQUIRE(cptr[0] == 0);
    for (int64_t u = 0; u < nu; ++u) {
        REQUIRE((size_t)cptr[(size_t)u] == want.size());
        for (int64_t k = 0; k < nf; ++k) {
            const dpg_factor& f = F[(size_t)k];
            if (u < n && f.i == u) want.push_back((int32_t)(k << 2 | 0));
            if (f.kind != DPG_FACTOR_BETWEEN) continue;
            if (u < n && f.j == u) want.push_back((int32_t)(k << 2 | 1));
            if (u >= n && pair[(size_t)k] == u - n) want.push_back((int32_t)(k << 2 | (f.i < f.j ? 2 : 3)));
        }
    }
    REQUIRE((size_t)cptr[(size_t)nu] == n_list && want == clist);
    return 0;
}

static int lists_checks() {
    const auto prior = [](int32_t i) { dpg_factor f; memset(&f, 0, sizeof(f)); f.kind = DPG_FACTOR_PRIOR; f.i = i; return f; };
    const auto between = [](int32_t i, int32_t j) {
        dpg_factor f;
        memset(&f, 0, sizeof(f));
        f.kind = DPG_FACTOR_BETWEEN;
        f.i = i;
        f.j = j;
        return f;
    };
    REQUIRE(lists_case(1, {prior(0)}, {}, {}) == 0);                         // one node, one prior
    REQUIRE(lists_case(2, {between(1, 0)}, {0}, {1}) == 0);                  // role 3
    REQUIRE(lists_case(2, {between(0, 1), prior(0), between(1, 0), prior(1)}, {0}, {1}) == 0);   // both orientations
    REQUIRE(lists_case(3, {}, {}, {}) == 0);                                 // no factors at all
    std::vector<dpg_factor> F = {prior(0)};                                  // 12-node chain, a closure every 4th node
    std::vector<int32_t> lo, hi;
    for (int32_t v = 1; v < 12; ++v) {
        F.push_back(between(v - 1, v));
        lo.push_back(v - 1);
        hi.push_back(v);
        if (v % 4 == 0) {
            F.push_back(between(v, v - 4));
            lo.push_back(v - 4);
            hi.push_back(v);
        }
    }
    REQUIRE(lists_case(12, F, lo, hi) == 0);
    printf("lists ok: 5 graphs\n");
    return 0;
}

// dpg_change_plan, the host half of dpg_execute_dpg_chain, against values worked out by hand.  No
// laser offset, resolution 0.05, every node's largest range 2, node v at (0.125 + 0.5 v, 0.125, 0):
// a chain node's rays need the keys [10 v - 37.5, 10 v + 42.5] x [-37.5, 42.5], widened by 4 cells
// (need) and, for a new window, by ceil(4 / 0.05) = 80 more on every side.
static bool same_kept(const ChangeKept& a, const ChangeKept& b) {
    return a.win.x0 == b.win.x0 && a.win.y0 == b.win.y0 && a.win.w == b.win.w && a.win.h == b.win.h && a.win_valid == b.win_valid &&
           memcmp(a.slot_node, b.slot_node, sizeof(a.slot_node)) == 0 && memcmp(a.slot_pose, b.slot_pose, sizeof(a.slot_pose)) == 0;
}
static bool same_ints(const int32_t* got, std::initializer_list<int32_t> want) { return std::equal(want.begin(), want.end(), got); }
static bool same_box(const Box& b, int32_t x0, int32_t y0, int32_t w, int32_t h) { return b.x0 == x0 && b.y0 == y0 && b.w == w && b.h == h; }

static int change_plan_checks() {
    dpg_change_params p;
    memset(&p, 0, sizeof(p));
    p.num_sectors = 5;
    p.current_pose_chain_len = 3;
    p.num_bins_for_change_detection = 36;
    p.occ_grid_resolution = 0.05;
    p.distance_threshold_for_local_submap_nodes = 5.0f;
    const int N = 20;
    std::vector<float> est(3 * N, 0.f), rmax(N, 2.0f);
    std::vector<uint8_t> act(N, 1);
    for (int v = 0; v < N; ++v) { est[3 * v] = 0.125f + 0.5f * (float)v; est[3 * v + 1] = 0.125f; }
    ChangePlan pl;
    ChangeKept k0, k1, k2;
    // (a) three calls, one new node each: the window of the first is reused, the two surviving chain
    // nodes keep their planes, only the new node is rasterised
    REQUIRE(dpg_change_plan(p, 6, 3, est.data(), nullptr, act.data(), rmax.data(), k0, pl) == DPG_OK);
    REQUIRE(pl.n_chain == 3 && same_ints(pl.chain, {3, 4, 5}) && pl.cand.size() == 3 && same_ints(pl.cand.data(), {0, 1, 2}));
    REQUIRE(!pl.reuse && same_box(pl.need, -12, -42, 110, 90) && same_box(pl.win, -92, -122, 270, 250) && pl.chain_sep == 0);
    REQUIRE(same_ints(pl.slot, {0, 1, 2}) && pl.n_rast == 3 && same_ints(pl.rast, {0, 1, 2}) && pl.keep_mask == 0u && pl.chain_bits == 0x3fu);
    REQUIRE(pl.cframe[1][0] == 2.125f && pl.cframe[1][1] == 0.125f && pl.cframe[1][2] == 1.f && pl.cframe[1][3] == 0.f);
    REQUIRE(pl.kept.win_valid && same_ints(pl.kept.slot_node, {3, 4, 5, -1}) && pl.kept.slot_pose[2][0] == 2.625f && same_kept(k0, ChangeKept()));
    k1 = pl.kept;
    REQUIRE(dpg_change_plan(p, 7, 3, est.data(), nullptr, act.data(), rmax.data(), k1, pl) == DPG_OK);
    REQUIRE(pl.reuse && same_box(pl.need, -2, -42, 110, 90) && same_box(pl.win, -92, -122, 270, 250) && same_ints(pl.chain, {4, 5, 6}));
    REQUIRE(same_ints(pl.slot, {1, 2, 0}) && pl.n_rast == 1 && pl.rast[0] == 2 && pl.keep_mask == 0x3cu && pl.chain_bits == 0x3fu);
    REQUIRE(same_ints(pl.kept.slot_node, {6, 4, 5, -1}));
    k2 = pl.kept;
    REQUIRE(dpg_change_plan(p, 8, 3, est.data(), nullptr, act.data(), rmax.data(), k2, pl) == DPG_OK);
    REQUIRE(pl.reuse && same_box(pl.need, 8, -42, 110, 90) && same_ints(pl.slot, {2, 0, 1}) && pl.n_rast == 1 && pl.rast[0] == 2);
    REQUIRE(pl.keep_mask == 0x33u && pl.chain_bits == 0x3fu && same_ints(pl.kept.slot_node, {6, 7, 5, -1}));
    REQUIRE(pl.cand.size() == 5 && same_ints(pl.cand.data(), {0, 1, 2, 3, 4}));
    // (b) the second call again, node 5's chain pose one ulp off: its plane is released, it is rasterised again
    float cp[9];
    memcpy(cp, &est[12], sizeof(cp));
    cp[3] = nextafterf(cp[3], 100.f);
    REQUIRE(dpg_change_plan(p, 7, 3, est.data(), cp, act.data(), rmax.data(), k1, pl) == DPG_OK);
    REQUIRE(pl.reuse && pl.chain_sep == 1 && same_ints(pl.slot, {1, 0, 2}) && pl.n_rast == 2 && same_ints(pl.rast, {1, 2}));
    REQUIRE(pl.keep_mask == 0x0cu && pl.chain_bits == 0x3fu && same_ints(pl.kept.slot_node, {5, 4, 6, -1}) && pl.kept.slot_pose[0][0] == cp[3]);
    // (c) node 6 five metres further on: its box leaves the kept window, which is rebuilt
    std::vector<float> far = est;
    far[18] = 10.125f;
    REQUIRE(dpg_change_plan(p, 7, 3, far.data(), nullptr, act.data(), rmax.data(), k1, pl) == DPG_OK);
    REQUIRE(!pl.reuse && same_box(pl.need, -2, -42, 250, 90) && same_box(pl.win, -82, -122, 410, 250));
    REQUIRE(same_ints(pl.slot, {0, 1, 2}) && pl.n_rast == 3 && same_ints(pl.rast, {0, 1, 2}) && pl.keep_mask == 0u);
    REQUIRE(same_ints(pl.kept.slot_node, {4, 5, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}));
    // (d) a chain of 15: every plane used, each once
    p.current_pose_chain_len = 15;
    REQUIRE(dpg_change_plan(p, 20, 20, est.data(), nullptr, act.data(), rmax.data(), k0, pl) == DPG_OK);
    REQUIRE(pl.n_chain == 15 && pl.n_rast == 15 && pl.chain[0] == 5 && pl.chain[14] == 19 && pl.cand.empty() && pl.chain_bits == 0x3fffffffu);
    for (int k = 0; k < 15; ++k) REQUIRE(pl.slot[k] == k && pl.rast[k] == k && pl.kept.slot_node[k] == 5 + k);
    // (e) no current pass: an empty chain, no candidates, the kept state as it was
    REQUIRE(dpg_change_plan(p, 20, 0, est.data(), nullptr, act.data(), rmax.data(), k1, pl) == DPG_OK);
    REQUIRE(pl.n_chain == 0 && pl.n_rast == 0 && pl.cand.empty() && same_kept(pl.kept, k1));
    // (f) the two errors; the caller's kept state is read only
    p.current_pose_chain_len = 3;
    const ChangeKept before = k1;
    cp[3] = NAN;
    REQUIRE(dpg_change_plan(p, 7, 3, est.data(), cp, act.data(), rmax.data(), k1, pl) == DPG_ERR_ARG && same_kept(k1, before));
    std::vector<float> wide(N, 500.f);   // some 20000 x 20000 cells needed: above 2^28 with or without the margin
    REQUIRE(dpg_change_plan(p, 7, 3, est.data(), nullptr, act.data(), wide.data(), k1, pl) == DPG_ERR_SIZE && same_kept(k1, before));
    // (g) candidates of a chain at the origin: exactly at the threshold is taken (3-4-5), one ulp
    // beyond it is not, an inactive node inside the radius is not
    std::vector<float> g(3 * 8, 0.f);
    g[0] = 3.f; g[1] = 4.f;                           // node 0: sqrtf(9 + 16) = 5 <= 5
    g[3] = 1.f; g[4] = 1.f;                           // node 1: inside, inactive
    g[6] = 100.f;                                     // node 2: far
    g[9] = 3.f; g[10] = nextafterf(4.f, 5.f);         // node 3: sqrtf(25.000004) > 5
    g[12] = -3.f; g[13] = -4.f;                       // node 4: exactly 5 again
    act[1] = 0;
    REQUIRE(dpg_change_plan(p, 8, 3, g.data(), nullptr, act.data(), rmax.data(), k0, pl) == DPG_OK);
    REQUIRE(pl.cand.size() == 2 && same_ints(pl.cand.data(), {0, 4}) && same_ints(pl.chain, {5, 6, 7}));
    printf("change plan ok: reuse, released plane, rebuild, 15 planes, empty chain, errors, candidates\n");
    return 0;
}

int main() {
    REQUIRE(buffer_checks() == 0);
    REQUIRE(change_plan_checks() == 0);
    const int V = 24, NB = 720;
    const float W = 20.f, amin = (float)-M_PI, amax = (float)M_PI, rmax = 12.f;
    std::vector<float> segs(4 * 512);
    const int64_t ns = dpg_synth_world(7, W, segs.data(), 512);
    REQUIRE(ns > 4);
    std::vector<double> gt(3 * V);
    REQUIRE(dpg_synth_trajectory(7, V, segs.data(), ns, W, 1.0f, gt.data()) == DPG_OK);
    std::vector<float> ranges((size_t)V * NB);
    REQUIRE(dpg_synth_scans(gt.data(), V, segs.data(), ns, NB, amin, amax, rmax, 0.2f, 0.f, 0.f, 0.01f, 11, 2,
                            ranges.data()) == DPG_OK);
    // clouds: the ABI's host path and the oracle's must agree exactly
    std::vector<float> pts;
    std::vector<int64_t> off(V + 1, 0);
    for (int v = 0; v < V; ++v) {
        std::vector<float> a(2 * NB), b(2 * NB), d(2 * NB);
        const int64_t na = dpg_scan_to_cloud(&ranges[(size_t)v * NB], NB, amin, amax, rmax, 0.2f, 0.f, 0.f, a.data());
        const int64_t nb = oracle_scan_to_cloud(&ranges[(size_t)v * NB], NB, amin, amax, rmax, 0.2f, 0.f, 0.f, b.data());
        REQUIRE(na == nb && memcmp(a.data(), b.data(), sizeof(float) * 2 * (size_t)na) == 0);
        REQUIRE(dpg_downsample_cloud(a.data(), na, 5, d.data()) == oracle_downsample(a.data(), na, 5, d.data()));
        pts.insert(pts.end(), a.begin(), a.begin() + 2 * na);
        off[(size_t)v + 1] = off[(size_t)v] + na;
    }
    std::vector<float> est(3 * V);
    for (int v = 0; v < V; ++v)
        for (int q = 0; q < 3; ++q) est[(size_t)(3 * v + q)] = (float)(gt[(size_t)(3 * v + q)] - (q < 2 ? gt[(size_t)q] : 0.0));
    // batched ICP (successive + a few loop closures), both NN modes, one run_icp with covariance
    std::vector<int32_t> edges;
    for (int v = 1; v < V; ++v) { edges.push_back(v - 1); edges.push_back(v); }
    for (int v = 4; v < V; v += 5) { edges.push_back(v - 4); edges.push_back(v); }
    const int64_t E = (int64_t)edges.size() / 2;
    dpg_icp_params p;
    dpg_icp_params_default(&p);
    std::vector<dpg_icp_result> res((size_t)E), res2((size_t)E);
    std::vector<double> hess((size_t)E * 9);
    REQUIRE(oracle_icp_batch(pts.data(), off.data(), V, edges.data(), E, est.data(), &p, ORACLE_NN_GRID, 1, res.data(),
                             hess.data()) == 0);
    REQUIRE(oracle_icp_batch(pts.data(), off.data(), V, edges.data(), E, est.data(), &p, ORACLE_NN_BRUTE, 1, res2.data(),
                             nullptr) == 0);
    for (int64_t e = 0; e < E; ++e) REQUIRE(memcmp(&res[(size_t)e], &res2[(size_t)e], sizeof(dpg_icp_result)) == 0);
    {
        dpg_icp_result r;
        double cov[9], h[9];
        REQUIRE(oracle_run_icp(&pts[2 * (size_t)off[1]], off[2] - off[1], &pts[0], off[1], &est[3], &est[0], &p,
                               ORACLE_NN_GRID, &r, cov, h) == 0);
    }
    // factors: prior, odometry, ICP; Gauss-Newton
    std::vector<dpg_factor> F;
    dpg_factor f;
    memset(&f, 0, sizeof(f));
    f.kind = DPG_FACTOR_PRIOR;
    f.info[0] = f.info[1] = 25.0;
    f.info[2] = 44.4;
    F.push_back(f);
    for (int v = 1; v < V; ++v) {
        REQUIRE(dpg_odometry_factor(&est[(size_t)(3 * v - 3)], &est[(size_t)(3 * v)], v - 1, v, 0.4f, 0.4f, 0.4f, 0.4f, &f) ==
                DPG_OK);
        F.push_back(f);
    }
    for (int64_t e = 0; e < E; ++e) {
        dpg_icp_factor(&res[(size_t)e], edges[(size_t)(2 * e)], edges[(size_t)(2 * e + 1)], &p, &f);
        F.push_back(f);
    }
    std::vector<double> X(est.begin(), est.end());
    dpg_gn_params gp;
    dpg_gn_params_default(&gp);
    dpg_gn_stats st;
    REQUIRE(oracle_optimize_graph(X.data(), V, F.data(), (int64_t)F.size(), &gp, &st) == 0);
    REQUIRE(st.iterations > 0 && std::isfinite(st.final_error));
    // symbolic analysis: from scratch, then the incremental state grown node by node
    std::vector<int32_t> lo, hi;
    for (int64_t e = 0; e < E; ++e) {
        lo.push_back(std::min(edges[(size_t)(2 * e)], edges[(size_t)(2 * e + 1)]));
        hi.push_back(std::max(edges[(size_t)(2 * e)], edges[(size_t)(2 * e + 1)]));
    }
    dpg_chol_opts o{64, 0.3};
    dpg_chol_sym S;
    REQUIRE(dpg_chol_symbolic(V, lo.data(), hi.data(), (int64_t)lo.size(), &o, &S) == 0);
    dpg_chol_incsym I;
    REQUIRE(dpg_incsym_reset(&I, 8, lo.data(), hi.data(), 0) == 0);
    for (int v = 8; v < V; ++v) {
        dpg_incsym_append(&I, 1);
        for (size_t k = 0; k < lo.size(); ++k)
            if (hi[k] == v) dpg_incsym_add_edge(&I, lo[k], hi[k]);
        dpg_chol_sym S2;
        REQUIRE(dpg_incsym_derive(&I, &o, &S2) == 0);
    }
    // the GPU solver's host plans of larger graphs
    REQUIRE(plan_checks() == 0);
    // the 6x6 covariance sandwich from its 16 sums: a regular d2J_dX2 (the diagonal dominates the
    // couplings), then a singular one (no pairs, no sums: H = 0)
    {
        const double sm[16] = {3.0, -2.0, 90.0, 4.0, -1.0, 70.0, 5.0, 60.0, 6.0, -4.0, 300.0, 8.0, -2.0, 200.0, 9.0, 150.0};
        const double zero[16] = {0.0};
        double cov6[36];
        REQUIRE(dpg_cov6_from_sums(sm, 40, 40, cov6) == DPG_OK);
        for (int i = 0; i < 36; ++i) REQUIRE(std::isfinite(cov6[i]));
        REQUIRE(dpg_cov6_from_sums(zero, 0, 0, cov6) == DPG_ERR_NUMERIC);
        printf("cov6 ok: regular and singular sums\n");
    }
    // DPG change detection: pass 0 = the first half, pass 1 = the second half as a later pass
    dpg_change_params cp;
    memset(&cp, 0, sizeof(cp));
    cp.num_sectors = 5;
    cp.current_pose_chain_len = 5;
    cp.num_bins_for_change_detection = 36;
    cp.delta_change_threshold = 0.2;
    cp.current_pose_graph_coverage_threshold = 1.0;
    cp.occ_grid_resolution = 0.05;
    cp.minimum_percent_active_sectors = 0.5f;
    cp.distance_threshold_for_local_submap_nodes = 5.0f;
    cp.laser[0] = 0.2f;
    std::vector<int64_t> boff(V + 1);
    std::vector<float> geom(3 * V);
    for (int v = 0; v <= V; ++v) boff[(size_t)v] = (int64_t)v * NB;
    for (int v = 0; v < V; ++v) { geom[(size_t)(3 * v)] = amin; geom[(size_t)(3 * v + 1)] = amax; geom[(size_t)(3 * v + 2)] = rmax; }
    const int half = V / 2;
    oracle_dpg* D = oracle_dpg_create(half, boff.data(), ranges.data(), geom.data(), &cp);
    REQUIRE(D != nullptr);
    for (int v = half; v < V; ++v) {
        const int64_t o1[2] = {0, NB};
        REQUIRE(oracle_dpg_append(D, 1, o1, &ranges[(size_t)v * NB], &geom[(size_t)(3 * v)]) == 0);
        dpg_change_stats cs;
        REQUIRE(oracle_execute_dpg(D, v + 1, v - half + 1, est.data(), &cs) == 0);
    }
    std::vector<uint8_t> lab((size_t)V * NB), sec(V), act(V);
    oracle_dpg_fetch(D, lab.data(), sec.data(), act.data());
    int64_t cnt[4];
    const int64_t n = oracle_active_dynamic_points(D, V, est.data(), nullptr, 0, cnt);
    std::vector<float> mp(2 * (size_t)n + 2);
    REQUIRE(oracle_active_dynamic_points(D, V, est.data(), mp.data(), n, cnt) == n);
    oracle_dpg_destroy(D);
    // the contribution lists of the batch and the incremental graph
    REQUIRE(lists_checks() == 0);
    printf("sanitize check ok: %lld edges, %d GN iterations, %d supernodes, %lld map points\n", (long long)E,
           st.iterations, S.ns, (long long)n);
    return 0;
}
