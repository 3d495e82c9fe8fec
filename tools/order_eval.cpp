// order_eval.cpp -- compare fill-reducing orders for the GPU Cholesky on a pose graph (host only):
// minimum degree vs nested dissection (several leaf sizes).  For each: fill (blocks), factor Mflop,
// supernodes, elimination-tree levels, largest front and the critical-path estimate the fused DAG
// factorization schedules by (front_est_us, dpg_chol_plan.h, summed along the longest leaf-to-root
// path), plus the ordering time.
// usage: order_eval PAIRS.bin        (int32 n, int32 P, then P x (lo, hi))
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

#include <algorithm>
#include <vector>

#include "../dpg-slam_amd/csrc/dpg_chol.h"
#include "../dpg-slam_amd/csrc/dpg_chol_plan.h"

static double now_ms() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

static void report(const char* name, double ms, const dpg_chol_sym& S) {
    int64_t nnz = 0;
    for (int32_t s = 0; s < S.ns; ++s) {
        const int64_t k = S.sn_c0[(size_t)s + 1] - S.sn_c0[(size_t)s], r = S.sn_rows_ptr[(size_t)s + 1] - S.sn_rows_ptr[(size_t)s];
        nnz += k * (k - 1) / 2 + k * r;
    }
    const double crit = dpg_chol_critical_path_us(S);
    double work = 0.0;
    for (int32_t s = 0; s < S.ns; ++s) {
        const int32_t k = S.sn_c0[(size_t)s + 1] - S.sn_c0[(size_t)s];
        const int32_t r = (int32_t)(S.sn_rows_ptr[(size_t)s + 1] - S.sn_rows_ptr[(size_t)s]);
        work += dpg_chol::front_est_us(3 * (k + r), 3 * k, (int32_t)(S.child_ptr[(size_t)s + 1] - S.child_ptr[(size_t)s]));
    }
    printf("%-10s order %8.2f ms | fill %8lld blocks, %8.1f Mflop, %5d supernodes, %4d levels, max front %4d | "
           "critical path ~%7.0f us, work ~%8.0f us\n",
           name, ms, (long long)nnz, S.flops * 1e-6, S.ns, S.n_levels, S.max_front, crit, work);
}

// the fronts on the critical path (dpg_chol_critical_path_us's longest leaf-to-root path), root
// first: pivot columns k and rows below r (blocks), panels of kFNB scalar columns (0: a small front,
// factored whole in LDS), children, the model's estimate
static void path_fronts(const dpg_chol_sym& S) {
    std::vector<double> cp((size_t)S.ns, 0.0), est((size_t)S.ns, 0.0);
    int32_t far = -1;
    for (int32_t s = S.ns - 1; s >= 0; --s) {
        const int32_t k = S.sn_c0[(size_t)s + 1] - S.sn_c0[(size_t)s];
        const int32_t r = (int32_t)(S.sn_rows_ptr[(size_t)s + 1] - S.sn_rows_ptr[(size_t)s]);
        const int32_t p = S.sn_parent[(size_t)s];
        est[(size_t)s] = dpg_chol::front_est_us(3 * (k + r), 3 * k, (int32_t)(S.child_ptr[(size_t)s + 1] - S.child_ptr[(size_t)s]));
        cp[(size_t)s] = est[(size_t)s] + (p >= 0 ? cp[(size_t)p] : 0.0);
        if (far < 0 || cp[(size_t)s] >= cp[(size_t)far]) far = s;   // ties -> the lowest front
    }
    std::vector<int32_t> path;
    for (int32_t s = far; s >= 0; s = S.sn_parent[(size_t)s]) path.push_back(s);
    int32_t panels = 0, cols = 0;
    printf("critical path: %zu fronts, ~%.0f us\n   front     k     r  panels  children  est us\n", path.size(), cp[(size_t)far]);
    for (size_t i = path.size(); i-- > 0;) {
        const int32_t s = path[i];
        const int32_t k = S.sn_c0[(size_t)s + 1] - S.sn_c0[(size_t)s];
        const int32_t r = (int32_t)(S.sn_rows_ptr[(size_t)s + 1] - S.sn_rows_ptr[(size_t)s]);
        const int32_t nch = (int32_t)(S.child_ptr[(size_t)s + 1] - S.child_ptr[(size_t)s]);
        const int32_t np = dpg_chol::front_is_small(3 * (k + r), nch) ? 0 : (3 * k + dpg_chol::kFNB - 1) / dpg_chol::kFNB;
        panels += np;
        cols += k;
        printf("  %6d  %4d  %4d  %6d  %8d  %6.1f\n", s, k, r, np, nch, est[(size_t)s]);
    }
    printf("  path total: %d pivot columns, %d panels\n", cols, panels);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n, P;
    if (fread(&n, 4, 1, f) != 1 || fread(&P, 4, 1, f) != 1) return 2;
    std::vector<int32_t> lo((size_t)P), hi((size_t)P);
    for (int32_t q = 0; q < P; ++q)
        if (fread(&lo[(size_t)q], 4, 1, f) != 1 || fread(&hi[(size_t)q], 4, 1, f) != 1) return 2;
    fclose(f);
    printf("graph: %d nodes, %d pairs\n", n, P);
    dpg_chol_opts o{64, 0.3};
    {
        std::vector<int32_t> perm;
        std::vector<std::vector<int32_t>> pat;
        const double t = now_ms();
        dpg_chol_order(n, lo.data(), hi.data(), P, perm, pat);
        const double ms = now_ms() - t;
        dpg_chol_sym S;
        dpg_chol_sym_from_patterns(n, perm, pat, &o, &S);
        report("min-degree", ms, S);
    }
    for (int k = 0; k < 4; ++k) {   // the batch analysis' candidates (dpg_chol_symbolic picks the shortest path)
        static const int prm[4][3] = {{0, 5, 0}, {2, 4, 2}, {8, 4, 2}, {4, 5, 1}};
        // each multi-start rule plain and with its separators refined (1, 4, 8 passes)
        for (int refine : {0, 1, 4, 8}) {
            if (refine > 0 && prm[k][0] == 0) continue;
            std::vector<int32_t> perm;
            std::vector<std::vector<int32_t>> pat;
            const double t = now_ms();
            if (dpg_chol_order_nd_sep(n, lo.data(), hi.data(), P, 16, prm[k][0], prm[k][1], prm[k][2], k > 0, perm, pat, false,
                                      refine))
                return 3;
            const double ms = now_ms() - t;
            dpg_chol_sym S;
            if (dpg_chol_sym_from_patterns(n, perm, pat, &o, &S)) return 4;
            char name[32];
            if (refine > 0) snprintf(name, sizeof(name), "sep/%d+r%d", k, refine);
            else snprintf(name, sizeof(name), "sep/%d", k);
            report(name, ms, S);
            if (argc > 2) path_fronts(S);   // any second argument: every candidate's path
        }
    }
    {
        const double t = now_ms();
        dpg_chol_sym S;
        if (dpg_chol_symbolic(n, lo.data(), hi.data(), P, &o, &S)) return 5;
        report("batch-pick", now_ms() - t, S);
        path_fronts(S);
    }
    for (int leaf : {32, 64, 128, 256, 512}) {
        std::vector<int32_t> perm;
        std::vector<std::vector<int32_t>> pat;
        const double t = now_ms();
        if (dpg_chol_order_nd(n, lo.data(), hi.data(), P, leaf, perm, pat)) return 3;
        const double ms = now_ms() - t;
        dpg_chol_sym S;
        if (dpg_chol_sym_from_patterns(n, perm, pat, &o, &S)) return 4;
        char name[32];
        snprintf(name, sizeof(name), "nd/%d", leaf);
        report(name, ms, S);
    }
    return 0;
}
