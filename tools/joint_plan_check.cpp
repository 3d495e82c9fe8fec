// joint_plan_check -- the joint-marginal planner (dpg_chol_plan_joint_pairs / _nodes,
// dpg_chol_plan.cpp) against brute force, on the CPU: the kernels follow its tables without bounds
// checks.  Graphs: a chain, a small mesh, two components, a band graph; each under minimum degree
// and nested dissection.  For every distinct queried node the path, its length and the first
// front / row are recomputed from sn_parent / sn_c0; for every block the common part of the two
// paths (as ancestor sets) and its length; the W slices must not overlap and must stay inside the
// reported size; every output block must be written exactly once.
//   g++ -std=c++17 -fsanitize=address,undefined -pthread -o joint_plan_check tools/joint_plan_check.cpp
//       dpg-slam_amd/csrc/dpg_chol_sym.cpp dpg-slam_amd/csrc/dpg_chol_plan.cpp   (one command)
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <set>
#include <utility>
#include <vector>

#include "../dpg-slam_amd/csrc/dpg_chol.h"
#include "../dpg-slam_amd/csrc/dpg_chol_plan.h"
#include "../include/dpg_slam_c.h"

using namespace dpg_chol;

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++g_fail <= 20) {                         \
                printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                printf(__VA_ARGS__);                      \
                printf("\n");                             \
            }                                             \
        }                                                 \
    } while (0)

struct Graph {
    const char* name;
    int32_t n;
    std::vector<int32_t> lo, hi;
    void edge(int32_t a, int32_t b) { lo.push_back(std::min(a, b)); hi.push_back(std::max(a, b)); }
};

Graph chain(int32_t n) {
    Graph g{"chain", n, {}, {}};
    for (int32_t i = 0; i + 1 < n; ++i) g.edge(i, i + 1);
    return g;
}
Graph mesh(int32_t w, int32_t h) {
    Graph g{"mesh", w * h, {}, {}};
    for (int32_t y = 0; y < h; ++y)
        for (int32_t x = 0; x < w; ++x) {
            if (x + 1 < w) g.edge(y * w + x, y * w + x + 1);
            if (y + 1 < h) g.edge(y * w + x, (y + 1) * w + x);
            if (x + 1 < w && y + 1 < h) g.edge(y * w + x, (y + 1) * w + x + 1);
        }
    return g;
}
Graph two_components() {   // a chain of 6 and a ring of 9 with a chord, plus an isolated node
    Graph g{"two-components", 16, {}, {}};
    for (int32_t i = 0; i < 5; ++i) g.edge(i, i + 1);
    for (int32_t i = 0; i < 9; ++i) g.edge(6 + i, 6 + (i + 1) % 9);
    g.edge(6, 10);
    return g;
}
Graph band(int32_t n, int32_t b) {
    Graph g{"band", n, {}, {}};
    for (int32_t i = 0; i < n; ++i)
        for (int32_t j = i + 1; j < std::min(n, i + b + 1); ++j) g.edge(i, j);
    return g;
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
int32_t rnd(int32_t n) {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (int32_t)(g_rng % (uint64_t)n);
}

int32_t k3_of(const dpg_chol_sym& S, int32_t s) { return 3 * (S.sn_c0[(size_t)s + 1] - S.sn_c0[(size_t)s]); }

std::vector<int32_t> brute_path(const dpg_chol_sym& S, int32_t v) {
    std::vector<int32_t> p;
    int32_t s = -1;
    for (int32_t t = 0; t < S.ns; ++t)   // the front whose columns hold v's position
        if (S.pos[(size_t)v] >= S.sn_c0[(size_t)t] && S.pos[(size_t)v] < S.sn_c0[(size_t)t + 1]) s = t;
    for (; s >= 0; s = S.sn_parent[(size_t)s]) p.push_back(s);
    return p;
}

void check_plan(const char* what, const JointPlan& J, const dpg_chol_sym& S,
                const std::vector<std::pair<int32_t, int32_t>>& blocks /* (u, v) per PathPair, in order */) {
    const size_t nq = J.nodes.size();
    CHECK(J.queries.size() == nq && J.len.size() == nq && J.path_ptr.size() == nq + 1, "%s: table sizes", what);
    std::vector<int64_t> slot((size_t)S.n, -1);
    std::vector<std::pair<int64_t, int64_t>> iv;
    for (size_t q = 0; q < nq; ++q) {
        const int32_t v = J.nodes[q];
        CHECK(slot[(size_t)v] < 0, "%s: node %d queried twice", what, v);
        slot[(size_t)v] = (int64_t)q;
        const std::vector<int32_t> bp = brute_path(S, v);
        const int64_t b = J.path_ptr[q], e = J.path_ptr[q + 1];
        CHECK((size_t)(e - b) == bp.size(), "%s: node %d path of %lld fronts, brute force %zu", what, v, (long long)(e - b), bp.size());
        int64_t len = 0;
        for (size_t t = 0; t < bp.size() && (int64_t)t < e - b; ++t) {
            CHECK(J.path_sn[(size_t)b + t] == bp[t], "%s: node %d path front %zu", what, v, t);
            CHECK(J.path_len[(size_t)b + t] == k3_of(S, bp[t]), "%s: node %d path length %zu", what, v, t);
            len += k3_of(S, bp[t]);
        }
        CHECK(J.len[q] == len, "%s: node %d slice of %lld scalars, brute force %lld", what, v, (long long)J.len[q], (long long)len);
        CHECK(J.queries[q].sn == bp[0], "%s: node %d first front", what, v);
        CHECK(J.queries[q].row == 3 * (S.pos[(size_t)v] - S.sn_c0[(size_t)bp[0]]), "%s: node %d first row", what, v);
        CHECK(J.queries[q].row >= 0 && J.queries[q].row + 3 <= k3_of(S, bp[0]), "%s: node %d row outside its front", what, v);
        CHECK(bp.back() >= 0 && S.sn_parent[(size_t)bp.back()] < 0, "%s: node %d path does not end at a root", what, v);
        iv.push_back({J.queries[q].w_off, J.queries[q].w_off + 3 * len});
    }
    std::sort(iv.begin(), iv.end());
    for (size_t q = 0; q < iv.size(); ++q) {
        CHECK(iv[q].first >= 0 && iv[q].second <= J.w_total, "%s: a slice leaves the W buffer", what);
        if (q) CHECK(iv[q].first >= iv[q - 1].second, "%s: W slices overlap", what);
    }
    CHECK(J.pairs.size() == blocks.size(), "%s: %zu blocks planned, %zu asked", what, J.pairs.size(), blocks.size());
    std::vector<int> written((size_t)(J.out_total / 9 * 9 == J.out_total ? J.out_total : 0), 0);
    CHECK(!written.empty() || J.out_total == 0, "%s: output size %lld", what, (long long)J.out_total);
    for (size_t t = 0; t < J.pairs.size() && t < blocks.size(); ++t) {
        const PathPair& P = J.pairs[t];
        const int32_t u = std::min(blocks[t].first, blocks[t].second), v = std::max(blocks[t].first, blocks[t].second);
        const std::vector<int32_t> pu = brute_path(S, u), pv = brute_path(S, v);
        const std::set<int32_t> su(pu.begin(), pu.end());
        int64_t len = 0;
        size_t common = 0;
        for (int32_t s : pv)
            if (su.count(s)) { len += k3_of(S, s); ++common; }
        // the common fronts are the last `common` of both paths, in the same order
        for (size_t c = 0; c < common; ++c)
            CHECK(pu[pu.size() - 1 - c] == pv[pv.size() - 1 - c], "%s: block %zu: the common fronts are no suffix", what, t);
        CHECK(P.len == len, "%s: block %zu (%d, %d): suffix %d, brute force %lld", what, t, u, v, P.len, (long long)len);
        const int64_t qu = slot[(size_t)u], qv = slot[(size_t)v];
        CHECK(qu >= 0 && qv >= 0, "%s: block %zu: node without a query", what, t);
        if (qu < 0 || qv < 0) continue;
        CHECK(P.a == J.queries[(size_t)qu].w_off + 3 * (J.len[(size_t)qu] - len), "%s: block %zu: left suffix start", what, t);
        CHECK(P.b == J.queries[(size_t)qv].w_off + 3 * (J.len[(size_t)qv] - len), "%s: block %zu: right suffix start", what, t);
        CHECK(P.a >= 0 && P.a + 3 * len <= J.w_total && P.b >= 0 && P.b + 3 * len <= J.w_total, "%s: block %zu: suffix outside W", what, t);
        CHECK(P.o >= 0 || P.ot >= 0, "%s: block %zu goes nowhere", what, t);
        for (int which = 0; which < 2; ++which) {
            const int64_t o = which ? P.ot : P.o;
            if (o < 0) continue;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) {
                    const int64_t e = o + (int64_t)r * J.ld + c;
                    CHECK(e >= 0 && e < J.out_total, "%s: block %zu writes outside the output", what, t);
                    if (e >= 0 && e < (int64_t)written.size()) written[(size_t)e]++;
                }
        }
    }
    for (size_t e = 0; e < written.size(); ++e) CHECK(written[e] == 1, "%s: output element %zu written %d times", what, e, written[e]);
}

void run(const Graph& g, int32_t order, int32_t max_cols, double relax) {
    dpg_chol_opts o;
    o.order = order;
    o.max_supernode_cols = max_cols;
    o.relax_fraction = relax;
    dpg_chol_sym S;
    const int rc = dpg_chol_symbolic(g.n, g.lo.data(), g.hi.data(), (int64_t)g.lo.size(), &o, &S);
    CHECK(rc == 0, "%s: symbolic analysis failed (%d)", g.name, rc);
    if (rc) return;
    int32_t roots = 0;
    for (int32_t s = 0; s < S.ns; ++s) roots += S.sn_parent[(size_t)s] < 0;
    char what[128];
    snprintf(what, sizeof what, "%s n=%d order=%d cols=%d", g.name, g.n, order, max_cols);
    // pairs: random ones, both orientations, (i, i), repeats, the ends
    std::vector<int32_t> pairs;
    auto add = [&](int32_t a, int32_t b) { pairs.push_back(a % g.n); pairs.push_back(b % g.n); };   // (tiny graphs)
    for (int q = 0; q < 60; ++q) add(rnd(g.n), rnd(g.n));
    add(0, g.n - 1), add(g.n - 1, 0), add(3, 3), add(3, 3), add(0, 1), add(0, 1), add(1, 0);
    JointPlan J;
    const int64_t np = (int64_t)pairs.size() / 2;
    dpg_chol_plan_joint_pairs(J, S, pairs.data(), np);
    std::vector<std::pair<int32_t, int32_t>> blocks;
    for (int64_t q = 0; q < np; ++q) blocks.push_back({pairs[(size_t)(2 * q)], pairs[(size_t)(2 * q + 1)]});
    CHECK(J.ld == 3 && J.out_total == 9 * np, "%s: pairs output layout", what);
    for (int64_t q = 0; q < np && q < (int64_t)J.pairs.size(); ++q) {
        const PathPair& P = J.pairs[(size_t)q];
        const bool fwd = blocks[(size_t)q].first <= blocks[(size_t)q].second;
        CHECK((fwd ? P.o : P.ot) == 9 * q && (fwd ? P.ot : P.o) == -1, "%s: pair %lld output slot", what, (long long)q);
    }
    check_plan(what, J, S, blocks);
    int64_t longest = 0;
    for (int64_t l : J.len) longest = std::max(longest, l);
    // nodes: a list with a repeat, out of order (the plan is rebuilt in the same object)
    std::vector<int32_t> nodes = {g.n - 1, 0, rnd(g.n), 2 % g.n, rnd(g.n), 2 % g.n, rnd(g.n)};
    dpg_chol_plan_joint_nodes(J, S, nodes.data(), (int64_t)nodes.size());
    blocks.clear();
    for (size_t p = 0; p < nodes.size(); ++p)
        for (size_t q = p; q < nodes.size(); ++q) blocks.push_back({nodes[p], nodes[q]});
    const int64_t nn = (int64_t)nodes.size();
    CHECK(J.ld == 3 * nn && J.out_total == 9 * nn * nn, "%s: nodes output layout", what);
    check_plan(what, J, S, blocks);
    printf("%-40s fronts %4d roots %2d max_front %3d blocks (vectors in %s)  longest queried path %lld scalars\n", what, S.ns,
           roots, S.max_front, path_in_lds(S.max_front) ? "LDS" : "global memory", (long long)longest);
}

}  // namespace

int main() {
    const Graph gs[] = {chain(1), chain(2), chain(60), mesh(9, 7), two_components(), band(130, 70)};
    for (const Graph& g : gs)
        for (int32_t order : {DPG_ORDER_MD, DPG_ORDER_ND, DPG_ORDER_AUTO}) {
            run(g, order, 64, 0.3);
            run(g, order, 2, 0.0);
        }
    if (g_fail) {
        printf("joint plan check: %d failures\n", g_fail);
        return 1;
    }
    printf("joint plan check ok\n");
    return 0;
}
