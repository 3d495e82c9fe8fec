// nd_refine_check.cpp -- the nested dissection's vertex-separator refinement (dpg_chol_sym.cpp,
// nd_refine: node-based Fiduccia-Mattheyses moves after each split) on the smallest shapes at which
// it can go wrong; host only.
//   fat       a 24 x 24 grid handed two adjacent columns as its separator: the result separates,
//             is no larger than the input and at most 24 nodes, both sides >= N / bal
//   ladder    a 2 x 400 ladder (a route driven twice): the refined order's root separator is at
//             most 2 nodes
//   clique    a clique whose vertices carry pendant chains: no side emptied, the balance kept
//   repeat    a route-like graph of 3000 nodes: the same order twice, and the threaded form's
//             order and patterns equal the serial form's, for every refined rule
//   default   refine = 0 gives the order without the argument, and the order this graph had before
//             the refinement existed (its hash)
//   every order is checked to be a permutation of 0 .. n - 1
// usage: nd_refine_check  -> prints "ok" or the first failure
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <set>
#include <utility>
#include <vector>

#include "../dpg-slam_amd/csrc/dpg_chol.h"

namespace {

struct Graph {
    int32_t n = 0;
    std::vector<int32_t> lo, hi;
    void edge(int32_t a, int32_t b) { lo.push_back(std::min(a, b)); hi.push_back(std::max(a, b)); }
};

int fail(const char* what) {
    printf("FAIL %s\n", what);
    return 1;
}

bool is_perm(const std::vector<int32_t>& p, int32_t n) {
    if ((int32_t)p.size() != n) return false;
    std::vector<char> seen((size_t)n, 0);
    for (int32_t v : p) {
        if (v < 0 || v >= n || seen[(size_t)v]) return false;
        seen[(size_t)v] = 1;
    }
    return true;
}

// no edge joins side 0 and side 1
bool separates(const Graph& g, const std::vector<int32_t>& side) {
    for (size_t e = 0; e < g.lo.size(); ++e) {
        const int32_t a = side[(size_t)g.lo[e]], b = side[(size_t)g.hi[e]];
        if (a != 2 && b != 2 && a != b) return false;
    }
    return true;
}

// the largest connected component once the vertices marked in `gone` are removed
int32_t largest_component(const Graph& g, const std::vector<char>& gone) {
    std::vector<std::vector<int32_t>> adj((size_t)g.n);
    for (size_t e = 0; e < g.lo.size(); ++e) {
        adj[(size_t)g.lo[e]].push_back(g.hi[e]);
        adj[(size_t)g.hi[e]].push_back(g.lo[e]);
    }
    std::vector<char> seen(gone);
    int32_t best = 0;
    std::vector<int32_t> stack;
    for (int32_t s = 0; s < g.n; ++s) {
        if (seen[(size_t)s]) continue;
        int32_t cnt = 0;
        stack.assign(1, s);
        seen[(size_t)s] = 1;
        while (!stack.empty()) {
            const int32_t v = stack.back();
            stack.pop_back();
            ++cnt;
            for (int32_t u : adj[(size_t)v])
                if (!seen[(size_t)u]) { seen[(size_t)u] = 1; stack.push_back(u); }
        }
        best = std::max(best, cnt);
    }
    return best;
}

// a route with local and long loop closures (tools/nd_par_check.cpp's shape), from a generator
// defined here so that the graph is the same under every standard library
Graph route_graph(int32_t n, uint64_t seed) {
    uint64_t s = seed * 6364136223846793005ull + 1442695040888963407ull;
    auto next = [&](uint32_t m) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)((s >> 33) % m);
    };
    std::set<std::pair<int32_t, int32_t>> pairs;
    for (int32_t v = 0; v + 1 < n; ++v) pairs.insert({v, v + 1});
    for (int32_t k = 0; k < 3 * n; ++k) {
        const int32_t i = (int32_t)next((uint32_t)n);
        const int32_t j = k % 4 == 0 ? (int32_t)next((uint32_t)n) : std::min(n - 1, std::max(0, i + (int32_t)next(121) - 60));
        if (i != j) pairs.insert({std::min(i, j), std::max(i, j)});
    }
    Graph g;
    g.n = n;
    for (auto& p : pairs) g.edge(p.first, p.second);
    return g;
}

uint64_t hash_of(const std::vector<int32_t>& p) {
    uint64_t h = 1469598103934665603ull;
    for (int32_t v : p) h = (h ^ (uint64_t)(uint32_t)v) * 1099511628211ull;
    return h;
}

int order(const Graph& g, int32_t starts, int32_t bal, int32_t score, bool cover, bool par, int32_t refine,
          std::vector<int32_t>& perm, std::vector<std::vector<int32_t>>& pat) {
    return dpg_chol_order_nd_sep(g.n, g.lo.data(), g.hi.data(), (int64_t)g.lo.size(), 16, starts, bal, score, cover, perm,
                                 pat, par, refine);
}

int check_fat() {
    const int32_t W = 24, bal = 4;
    Graph g;
    g.n = W * W;
    for (int32_t r = 0; r < W; ++r)
        for (int32_t c = 0; c < W; ++c) {
            if (c + 1 < W) g.edge(r * W + c, r * W + c + 1);
            if (r + 1 < W) g.edge(r * W + c, (r + 1) * W + c);
        }
    for (int32_t score : {0, 1, 2}) {
        std::vector<int32_t> side((size_t)g.n);
        for (int32_t r = 0; r < W; ++r)
            for (int32_t c = 0; c < W; ++c) side[(size_t)(r * W + c)] = c < 11 ? 0 : c > 12 ? 1 : 2;
        if (dpg_chol_nd_refine(g.n, g.lo.data(), g.hi.data(), (int64_t)g.lo.size(), bal, score, 4, side)) return fail("fat: rc");
        int32_t cnt[3] = {0, 0, 0};
        for (int32_t s : side) {
            if (s < 0 || s > 2) return fail("fat: side value");
            cnt[s]++;
        }
        if (!separates(g, side)) return fail("fat: an edge joins the sides");
        if (cnt[2] > 2 * W || cnt[2] > W) return fail("fat: separator too large");
        if (bal * cnt[0] < g.n || bal * cnt[1] < g.n) return fail("fat: balance");
    }
    return 0;
}

int check_ladder() {
    const int32_t L = 400, bal = 4;
    Graph g;
    g.n = 2 * L;
    for (int32_t i = 0; i < L; ++i) {
        if (i + 1 < L) { g.edge(i, i + 1); g.edge(L + i, L + i + 1); }
        g.edge(i, L + i);
    }
    for (bool par : {false, true}) {
        std::vector<int32_t> perm;
        std::vector<std::vector<int32_t>> pat;
        if (order(g, 8, bal, 2, true, par, 4, perm, pat) || !is_perm(perm, g.n)) return fail("ladder: order");
        // the root separator is the end of the order: its last k <= 2 nodes must split the ladder
        // into parts that each leave the other side N / bal
        bool ok = false;
        for (int32_t k = 1; k <= 2 && !ok; ++k) {
            std::vector<char> gone((size_t)g.n, 0);
            for (int32_t t = 0; t < k; ++t) gone[(size_t)perm[(size_t)(g.n - 1 - t)]] = 1;
            ok = bal * (g.n - k - largest_component(g, gone)) >= g.n;
        }
        if (!ok) return fail("ladder: root separator larger than 2 nodes");
    }
    return 0;
}

int check_clique() {
    const int32_t K = 10, C = 5, bal = 4;   // K clique vertices, each with a chain of C pendant nodes
    Graph g;
    g.n = K * (1 + C);
    for (int32_t a = 0; a < K; ++a) {
        for (int32_t b = a + 1; b < K; ++b) g.edge(a, b);
        for (int32_t c = 0; c < C; ++c) g.edge(c == 0 ? a : K + a * C + c - 1, K + a * C + c);
    }
    for (int32_t score : {0, 2}) {
        std::vector<int32_t> side((size_t)g.n, 2);   // the clique separates the chains
        for (int32_t a = 0; a < K; ++a)
            for (int32_t c = 0; c < C; ++c) side[(size_t)(K + a * C + c)] = a < K / 2 ? 0 : 1;
        if (dpg_chol_nd_refine(g.n, g.lo.data(), g.hi.data(), (int64_t)g.lo.size(), bal, score, 4, side)) return fail("clique: rc");
        int32_t cnt[3] = {0, 0, 0};
        for (int32_t s : side) cnt[s]++;
        if (!separates(g, side)) return fail("clique: an edge joins the sides");
        if (cnt[0] == 0 || cnt[1] == 0) return fail("clique: a side emptied");
        if (bal * cnt[0] < g.n || bal * cnt[1] < g.n) return fail("clique: balance");
        if (cnt[2] > K) return fail("clique: separator grew");
    }
    std::vector<int32_t> perm;
    std::vector<std::vector<int32_t>> pat;
    if (order(g, 8, bal, 2, true, false, 4, perm, pat) || !is_perm(perm, g.n)) return fail("clique: order");
    return 0;
}

int check_repeat_and_default() {
    const Graph g = route_graph(3000, 7);
    const struct { int32_t starts, bal, score; bool cover; } rules[] = {
        {8, 4, 2, true}, {8, 4, 0, true}, {16, 5, 2, true}, {4, 5, 1, false}};
    for (auto& r : rules) {
        std::vector<int32_t> p0, p1, p2;
        std::vector<std::vector<int32_t>> t0, t1, t2;
        if (order(g, r.starts, r.bal, r.score, r.cover, false, 4, p0, t0) || order(g, r.starts, r.bal, r.score, r.cover, false, 4, p1, t1) ||
            order(g, r.starts, r.bal, r.score, r.cover, true, 4, p2, t2))
            return fail("repeat: order");
        if (!is_perm(p0, g.n)) return fail("repeat: not a permutation");
        if (p0 != p1 || t0 != t1) return fail("repeat: two runs differ");
        if (p0 != p2 || t0 != t2) return fail("repeat: threaded form differs from the serial form");
        // refine = 0: the order without the argument
        std::vector<int32_t> q0, q1;
        std::vector<std::vector<int32_t>> u0, u1;
        if (order(g, r.starts, r.bal, r.score, r.cover, false, 0, q0, u0) ||
            dpg_chol_order_nd_sep(g.n, g.lo.data(), g.hi.data(), (int64_t)g.lo.size(), 16, r.starts, r.bal, r.score, r.cover, q1, u1))
            return fail("default: order");
        if (!is_perm(q0, g.n) || q0 != q1 || u0 != u1) return fail("default: refine = 0 differs from the plain call");
    }
    // the unrefined orders of this graph as they were before the refinement existed
    const struct { int32_t starts, bal, score; bool cover; uint64_t hash; } before[] = {
        {0, 5, 0, false, 17497643003303416057ull}, {8, 4, 2, true, 15910292896370157623ull}};
    for (auto& b : before) {
        std::vector<int32_t> p;
        std::vector<std::vector<int32_t>> t;
        if (order(g, b.starts, b.bal, b.score, b.cover, false, 0, p, t)) return fail("default: order");
        if (hash_of(p) != b.hash) {
            printf("FAIL default: starts %d hash %llu\n", b.starts, (unsigned long long)hash_of(p));
            return 1;
        }
    }
    return 0;
}

}  // namespace

int main() {
    if (check_fat() || check_ladder() || check_clique() || check_repeat_and_default()) return 1;
    printf("ok\n");
    return 0;
}
