// dpg_store.hip -- the DPG node store (dpg_dpg.h): creation, append, release, read-back and reload,
// the device view the kernels take (make_ds) and the cache of node frames.  No kernel lives here.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dpg_dpg.h"

namespace {

// beams per scan of n nodes with the offsets off[0 .. n]; *max_beams grows to the largest
int check_beams(int64_t n, const int64_t* off, int32_t* max_beams) {
    for (int64_t k = 0; k < n; ++k) {
        const int64_t nb = off[k + 1] - off[k];
        if (nb < 2 || nb > 65535) return fail(DPG_ERR_SIZE, "beams per scan must be in [2, 65535]");
        *max_beams = std::max<int32_t>(*max_beams, (int32_t)nb);
    }
    return DPG_OK;
}

// createNode (dpg_slam.cc:497-507) and MeasurementPoint (dpg_measurement.h:41-46,102-104) for n nodes:
// node k's beams are ranges[off[k] - base ..), its geometry geom[3 k ..) = amin, amax, rmax.  Per beam
// the laser-frame point, label and sector; per node geom4 = amin, amax, rmax, angle_inc and the largest range.
void derive_nodes(int64_t n, const int64_t* off, int64_t base, const float* ranges, const float* geom, int32_t num_sectors,
                  float2* pl, uint8_t* lab, uint8_t* sec, float* geom4, float* rmax_beam) {
    for (int64_t k = 0; k < n; ++k) {
        const int64_t nb = off[k + 1] - off[k];
        const float amin = geom[3 * k], amax = geom[3 * k + 1], rmax = geom[3 * k + 2];
        const float ainc = (float)((double)(amax - amin) / ((double)nb - 1.0));
        const float per_sector = ((float)nb) / (float)num_sectors;
        geom4[4 * k] = amin; geom4[4 * k + 1] = amax; geom4[4 * k + 2] = rmax; geom4[4 * k + 3] = ainc;
        float rm = 0.f;
        for (int64_t i = 0; i < nb; ++i) {
            const int64_t b = off[k] - base + i;
            const float angle = ainc * (float)i + amin;
            const float r = ranges[b];
            pl[b] = make_float2(r * cosf(angle), r * sinf(angle));
            lab[b] = r >= rmax ? DPG_LABEL_MAX_RANGE : DPG_LABEL_NOT_YET_LABELED;
            sec[b] = (uint8_t)((float)i / per_sector);
            rm = std::max(rm, r);
        }
        rmax_beam[k] = rm;
    }
}

}  // namespace

DS make_ds(dpg_dpg* d) {
    DS s;
    memset(&s, 0, sizeof(s));
    const int32_t* stage = d->d_stage.p;
    s.off = d->d_off.p; s.plaser = d->d_plaser.p; s.range = d->d_range.p; s.label = d->d_label.p;
    s.sector = d->d_sector.p; s.geom = d->d_geom.p; s.sect = d->d_sect.p; s.active = d->d_active.p;
    s.frame = d->d_frame.p; s.grid = d->d_grid.p; s.first = d->d_first.p;
    if (stage) {
        s.chain = stage + kStageChain; s.slot = stage + kStageSlot; s.rast = stage + kStageRast;
        s.cframe = reinterpret_cast<const float4*>(stage + kStageFrames); s.cand = stage + kStageCand;
    }
    s.cand_cnt = d->d_cand_cnt.p; s.acc = d->d_acc.p; s.bins = d->d_bins.p;
    s.inrange = d->d_inrange.p; s.commit = d->d_commit.p; s.added = d->d_added.p; s.rmask = d->d_rmask.p;
    s.removed_xy = d->d_removed.p; s.ctl = d->d_ctl.p;
    s.res = d->p.occ_grid_resolution; s.inv_res = 1.0 / d->p.occ_grid_resolution; s.max_beams = d->max_beams; s.num_sectors = d->p.num_sectors;
    s.total_bins = d->p.num_bins_for_change_detection; s.bin_words = (d->p.num_bins_for_change_detection + 2 + 31) / 32;
    s.min_pct = d->p.minimum_percent_active_sectors; s.change_thr = d->p.delta_change_threshold;
    s.cover_thr = d->p.current_pose_graph_coverage_threshold;
    return s;
}

int upload_frames(dpg_dpg* d, int64_t V, const float* est, bool active_only) {
    int64_t lo = V, hi = -1;
    for (int64_t v = 0; v < V; ++v) {
        if (active_only && !d->active_h[(size_t)v]) continue;
        float* c = &d->h_pose[(size_t)(3 * v)];
        if (memcmp(c, est + 3 * v, 3 * sizeof(float)) == 0) continue;
        memcpy(c, est + 3 * v, 3 * sizeof(float));
        node_frame(d->p.laser, est + 3 * v, &d->h_frames.p[(size_t)(8 * v)]);
        lo = std::min(lo, v);
        hi = v;
    }
    if (hi >= lo)
        HIP_TRY(hipMemcpyAsync(d->d_frame.p + 2 * lo, &d->h_frames.p[(size_t)(8 * lo)], sizeof(float) * 8 * (hi - lo + 1),
                               hipMemcpyHostToDevice, d->s));
    return DPG_OK;
}

extern "C" {

void dpg_change_params_default(dpg_change_params* p) {
    memset(p, 0, sizeof(*p));
    p->num_sectors = 5; p->current_pose_chain_len = 5; p->num_bins_for_change_detection = 36;
    p->delta_change_threshold = 0.20; p->current_pose_graph_coverage_threshold = 1.0;
    p->occ_grid_resolution = 0.05; p->minimum_percent_active_sectors = 0.5f;
    p->distance_threshold_for_local_submap_nodes = 5.0f;
    p->laser[0] = 0.2f; p->laser[1] = 0.f; p->laser[2] = 0.f;
}

dpg_dpg* dpg_dpg_create(dpg_ctx* ctx, int64_t V, const int64_t* off, const float* ranges, const float* geom,
                        const dpg_change_params* p) {
    if (!ctx || V <= 0 || !off || !ranges || !geom || !p) { fail(DPG_ERR_ARG, "bad arguments"); return nullptr; }
    if (p->num_sectors < 1 || p->num_sectors > 8 || p->current_pose_chain_len < 0 || p->current_pose_chain_len > kChainMax ||
        p->num_bins_for_change_detection < 1 || p->num_bins_for_change_detection > 65534 || !(p->occ_grid_resolution > 0)) {
        fail(DPG_ERR_ARG, "change params out of range (sectors 1..8, chain 0..15, bins 1..65534, resolution > 0)");
        return nullptr;
    }
    int32_t max_beams = 0;
    if (check_beams(V, off, &max_beams)) return nullptr;
    dpg_dpg* d = new dpg_dpg();
    d->ctx = ctx; d->s = ctx->stream; d->device = ctx->device; d->p = *p;
    d->V = V; d->B = off[V]; d->max_beams = max_beams;
    d->off.assign(off, off + V + 1);
    d->geom.resize((size_t)(4 * V));
    d->rmax_beam.assign((size_t)V, 0.f);
    d->active_h.assign((size_t)V, 1);
    d->h_pose.assign((size_t)(3 * V), NAN);
    std::vector<float2> pl((size_t)d->B);
    std::vector<uint8_t> lab((size_t)d->B), sec((size_t)d->B);
    derive_nodes(V, off, 0, ranges, geom, p->num_sectors, pl.data(), lab.data(), sec.data(), d->geom.data(), d->rmax_beam.data());
    std::vector<uint32_t> sect((size_t)V, (1u << p->num_sectors) - 1u), act((size_t)V, 1u);
    // error paths: d's buffers and events release themselves
    auto bad = [&](const char* m) { dpg_dpg_destroy(d); fail(DPG_ERR_HIP, "%s", m); return (dpg_dpg*)nullptr; };
    if (hipSetDevice(d->device) != hipSuccess) return bad("hipSetDevice failed");
    if (d->d_off.reserve((size_t)(V + 1)) || d->d_plaser.reserve((size_t)d->B) || d->d_range.reserve((size_t)d->B) ||
        d->d_label.reserve((size_t)d->B) || d->d_sector.reserve((size_t)d->B) || d->d_geom.reserve((size_t)V) ||
        d->d_sect.reserve((size_t)V) || d->d_active.reserve((size_t)V) || d->d_ctl.reserve(1) ||
        d->d_frame.reserve((size_t)(2 * V)))
        return bad("hipMalloc failed");
    if (d->h_ctl.reserve(1) || d->h_frames.reserve((size_t)(8 * V)) || d->h_act.reserve((size_t)V) || d->h_commit.reserve(16))
        return bad("hipHostMalloc failed");
    memset(d->h_frames.p, 0, sizeof(float) * 8 * V);
    hipStream_t s = d->s;
    if (hipMemcpyAsync(d->d_off.p, off, sizeof(int64_t) * (V + 1), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d->d_plaser.p, pl.data(), sizeof(float2) * d->B, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d->d_range.p, ranges, sizeof(float) * d->B, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d->d_label.p, lab.data(), d->B, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d->d_sector.p, sec.data(), d->B, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d->d_geom.p, d->geom.data(), sizeof(float) * 4 * V, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d->d_sect.p, sect.data(), sizeof(uint32_t) * V, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d->d_active.p, act.data(), sizeof(uint32_t) * V, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return bad("upload of the node store failed");
    for (auto& e : d->ev) (void)e.ensure(hipEventDefault);
    dpg_ctx_adopt(ctx, d, [](void* x) { dpg_dpg_destroy(static_cast<dpg_dpg*>(x)); });
    return d;
}

// One node per call on the DpgSLAM path: the cost is per call, so nothing here is O(V) -- the
// device arrays and the pinned mirrors grow by 1.5x with their contents kept, the new nodes' data
// are built straight into one pinned staging block and go up from it (only the new offsets, not
// the whole offset array), and the stream is not waited on at the end (the next call, or any
// executeDPG, is queued behind these copies; the staging block is reused only after the stream
// synchronisation that opens the next call).
int dpg_dpg_append(dpg_dpg* d, int64_t n_new, const int64_t* off_rel, const float* ranges, const float* geom) {
    if (!d || n_new < 0 || (n_new > 0 && (!off_rel || !ranges || !geom))) return fail(DPG_ERR_ARG, "bad arguments");
    if (n_new == 0) return DPG_OK;
    HIP_TRY(hipSetDevice(d->device));
    hipStream_t s = d->s;
    HIP_TRY(hipStreamSynchronize(s));
    const int64_t V0 = d->V, B0 = d->B, V1 = V0 + n_new, nb_new = off_rel[n_new] - off_rel[0];
    int32_t max_beams = d->max_beams;
    int rc = check_beams(n_new, off_rel, &max_beams);
    if (rc) return rc;
    // staging layout (16-B aligned parts): offsets [n_new] i64 | plaser [nb] float2 | range [nb] f32 |
    // geom [n_new] float4 | sect [n_new] u32 | active [n_new] u32 | label [nb] u8 | sector [nb] u8
    auto al = [](size_t x) { return (x + 15) & ~size_t(15); };
    const size_t o_off = 0, o_pl = al(o_off + 8 * (size_t)n_new), o_rg = al(o_pl + 8 * (size_t)nb_new),
                 o_gm = al(o_rg + 4 * (size_t)nb_new), o_sc = al(o_gm + 16 * (size_t)n_new),
                 o_ac = al(o_sc + 4 * (size_t)n_new), o_lb = al(o_ac + 4 * (size_t)n_new), o_sr = al(o_lb + (size_t)nb_new),
                 need = al(o_sr + (size_t)nb_new);
    if (d->h_app.grow(need, 0, s)) return fail(DPG_ERR_HIP, "hipHostMalloc(append staging) failed");
    unsigned char* st = d->h_app.p;
    int64_t* off_new = reinterpret_cast<int64_t*>(st + o_off);
    float2* pl = reinterpret_cast<float2*>(st + o_pl);
    float* rg = reinterpret_cast<float*>(st + o_rg);
    float* gm = reinterpret_cast<float*>(st + o_gm);
    uint32_t* sect = reinterpret_cast<uint32_t*>(st + o_sc);
    uint32_t* act = reinterpret_cast<uint32_t*>(st + o_ac);
    uint8_t *lab = st + o_lb, *sec = st + o_sr;
    // the new nodes' largest ranges and the beam maximum are committed to d only after every
    // allocation and copy below succeeded (as off and V)
    std::vector<float> rmax_new((size_t)n_new);
    derive_nodes(n_new, off_rel, off_rel[0], ranges, geom, d->p.num_sectors, pl, lab, sec, gm, rmax_new.data());
    memcpy(rg, ranges, sizeof(float) * (size_t)nb_new);
    for (int64_t k = 0; k < n_new; ++k) {
        off_new[k] = d->off.back() + (off_rel[k + 1] - off_rel[0]);
        sect[k] = (1u << d->p.num_sectors) - 1u;
        act[k] = 1u;
    }
    // device arrays grow with their contents kept (amortised x1.5)
    const size_t B1 = (size_t)(B0 + nb_new);
    if (d->d_off.grow((size_t)(V1 + 1), (size_t)(V0 + 1), s) || d->d_plaser.grow(B1, (size_t)B0, s) ||
        d->d_range.grow(B1, (size_t)B0, s) || d->d_label.grow(B1, (size_t)B0, s) || d->d_sector.grow(B1, (size_t)B0, s) ||
        d->d_geom.grow((size_t)V1, (size_t)V0, s) || d->d_sect.grow((size_t)V1, (size_t)V0, s) ||
        d->d_active.grow((size_t)V1, (size_t)V0, s) || d->d_frame.grow((size_t)(2 * V1), (size_t)(2 * V0), s))
        return fail(DPG_ERR_HIP, "hipMalloc(node store growth) failed");
    // pinned host mirrors, amortised x1.5 (the activity mirror is rewritten by every call)
    if (d->h_frames.grow((size_t)(8 * V1), (size_t)(8 * V0), s) || d->h_act.grow((size_t)V1, 0, s))
        return fail(DPG_ERR_HIP, "hipHostMalloc(node store growth) failed");
    memset(d->h_frames.p + 8 * V0, 0, sizeof(float) * 8 * n_new);
    HIP_TRY(hipMemcpyAsync(d->d_off.p + V0 + 1, off_new, sizeof(int64_t) * n_new, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d->d_plaser.p + B0, pl, sizeof(float2) * nb_new, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d->d_range.p + B0, rg, sizeof(float) * nb_new, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d->d_label.p + B0, lab, nb_new, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d->d_sector.p + B0, sec, nb_new, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d->d_geom.p + V0, gm, sizeof(float) * 4 * n_new, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d->d_sect.p + V0, sect, sizeof(uint32_t) * n_new, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d->d_active.p + V0, act, sizeof(uint32_t) * n_new, hipMemcpyHostToDevice, s));
    d->h_pose.resize((size_t)(3 * V1), NAN);
    d->active_h.resize((size_t)V1, 1);
    d->geom.insert(d->geom.end(), gm, gm + 4 * n_new);
    d->off.insert(d->off.end(), off_new, off_new + n_new);
    d->V = V1; d->B = (int64_t)B1;
    d->rmax_beam.insert(d->rmax_beam.end(), rmax_new.begin(), rmax_new.end());
    d->max_beams = max_beams;
    return DPG_OK;
}

void dpg_dpg_destroy(dpg_dpg* d) {
    if (!d) return;
    dpg_ctx_release_child(d->ctx, d);
    (void)hipSetDevice(d->device);
    (void)hipStreamSynchronize(d->s);
    delete d;
}

int dpg_dpg_fetch(dpg_dpg* d, uint8_t* labels, uint8_t* sector_active, uint8_t* node_active) {
    if (!d) return fail(DPG_ERR_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipStreamSynchronize(d->s));
    if (labels) HIP_TRY(hipMemcpy(labels, d->d_label.p, d->B, hipMemcpyDeviceToHost));
    std::vector<uint32_t> t((size_t)d->V);
    if (sector_active) {
        HIP_TRY(hipMemcpy(t.data(), d->d_sect.p, sizeof(uint32_t) * d->V, hipMemcpyDeviceToHost));
        for (int64_t v = 0; v < d->V; ++v) sector_active[v] = (uint8_t)t[(size_t)v];
    }
    if (node_active) {
        HIP_TRY(hipMemcpy(t.data(), d->d_active.p, sizeof(uint32_t) * d->V, hipMemcpyDeviceToHost));
        for (int64_t v = 0; v < d->V; ++v) node_active[v] = t[(size_t)v] ? 1 : 0;
    }
    return DPG_OK;
}

int dpg_dpg_load(dpg_dpg* d, const uint8_t* labels, const uint8_t* sector_active, const uint8_t* node_active) {
    if (!d) return fail(DPG_ERR_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipStreamSynchronize(d->s));
    d->kept.win_valid = false;   // the kept chain planes may no longer match the node state
    if (labels) HIP_TRY(hipMemcpy(d->d_label.p, labels, d->B, hipMemcpyHostToDevice));
    std::vector<uint32_t> t((size_t)d->V);
    if (sector_active) {
        const uint32_t full = (1u << d->p.num_sectors) - 1u;
        for (int64_t v = 0; v < d->V; ++v) t[(size_t)v] = sector_active[v] & full;
        HIP_TRY(hipMemcpy(d->d_sect.p, t.data(), sizeof(uint32_t) * d->V, hipMemcpyHostToDevice));
    }
    if (node_active) {
        for (int64_t v = 0; v < d->V; ++v) { t[(size_t)v] = node_active[v] ? 1u : 0u; d->active_h[(size_t)v] = node_active[v] ? 1 : 0; }
        HIP_TRY(hipMemcpy(d->d_active.p, t.data(), sizeof(uint32_t) * d->V, hipMemcpyHostToDevice));
    }
    return DPG_OK;
}

}  // extern "C"
