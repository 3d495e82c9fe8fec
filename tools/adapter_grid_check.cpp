// adapter_grid_check.cpp -- DpgStore::occupancyGrid of include/dpg_slam_adapter.hpp with a stand-in
// for DpgNode: compiled and linked against lib/libdpg.so by the CPU suite
// (tests/test_occupancy_grid_cpu.py), run on the GPU by tests/test_occupancy_grid.py.  The adapter's
// grid is checked against the direct C-ABI call on the same state, byte for byte, and against the
// host formula (dpg_occupancy_from_counts) over the C call's counters.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <utility>
#include <vector>

#include "../include/dpg_slam_adapter.hpp"

namespace {

struct Vector2f {
    float v[2];
    Vector2f(float a = 0.f, float b = 0.f) : v{a, b} {}
    float x() const { return v[0]; }
    float y() const { return v[1]; }
};
struct Node {
    Vector2f loc;
    float th = 0.f;
    std::pair<Vector2f, float> getEstimatedPosition() const { return {loc, th}; }
};

int fails = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++fails; } \
    } while (0)

}  // namespace

int main() {
    dpg_adapter::Context ctx(0);
    dpg_adapter::DpgStore store(ctx.get());
    std::vector<Node> nodes(2);
    nodes[0].loc = Vector2f(-3.25f, 1.5f);
    nodes[0].th = 0.3f;
    nodes[1].loc = Vector2f(-2.5f, 1.0f);
    nodes[1].th = -2.1f;
    std::vector<float> r0(360, 5.0f), r1(360, 5.0f);
    for (int b = 0; b < 72; ++b) r1[(size_t)b] = 7.0f;
    store.add_scan(r0, (float)-M_PI, (float)M_PI, 8.f);
    store.add_scan(r1, (float)-M_PI, (float)M_PI, 8.f);
    for (const double res : {0.0, 0.1}) {
        std::vector<int8_t> data;
        dpg_grid_info info;
        store.occupancyGrid(nodes, res, data, info);
        const int64_t cells = (int64_t)info.w * info.h;
        EXPECT(cells > 0 && (int64_t)data.size() == cells && info.n_oob == 0 && info.n_nodes_used == 2);
        EXPECT(info.resolution == (res == 0.0 ? 0.05 : res));
        float est[6];
        for (size_t i = 0; i < 2; ++i) dpg_adapter::pose_of(nodes[i], &est[3 * i]);
        dpg_grid_params gp;
        dpg_grid_params_default(&gp);
        gp.resolution = res;
        std::vector<int32_t> hits((size_t)cells), misses((size_t)cells);
        std::vector<int8_t> occ((size_t)cells), host((size_t)cells);
        dpg_grid_info direct;
        EXPECT(dpg_occupancy_grid(store.get(), 2, est, &gp, hits.data(), misses.data(), occ.data(), cells, &direct) == DPG_OK);
        EXPECT(direct.x0 == info.x0 && direct.y0 == info.y0 && direct.w == info.w && direct.h == info.h);
        EXPECT(memcmp(occ.data(), data.data(), (size_t)cells) == 0);
        dpg_occupancy_from_counts(hits.data(), misses.data(), cells, host.data());
        EXPECT(memcmp(host.data(), data.data(), (size_t)cells) == 0);
        int64_t known = 0;
        for (int64_t c = 0; c < cells; ++c) known += data[(size_t)c] >= 0;
        EXPECT(known > 0 && direct.n_hits > 0);
        printf("occupancyGrid res %.2f: %d x %d cells at (%d, %d), %lld known, %lld hits, %lld samples\n", info.resolution,
               info.w, info.h, info.x0, info.y0, (long long)known, (long long)direct.n_hits, (long long)direct.n_samples);
    }
    printf(fails ? "adapter grid check FAILED (%d)\n" : "adapter grid check ok\n", fails);
    return fails ? 1 : 0;
}
