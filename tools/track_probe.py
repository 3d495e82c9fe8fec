"""Frozen-map probe, on the node store of the `--workload dpg` benchmark that
tools/loc_probe.py uses (config 5: passes of 2500 nodes of a 64 m building, 5000-beam 270-degree 30 m
scans, 48 movable boxes, ground-truth poses).  The map is pass 0 with every node active, frozen at
0.05 m; the scans are the first of pass 1, every --ratio-th point of each.

Each figure: one uncounted call, then the median of --calls calls, of the HIP-event time of the
kernels and of the wall time of the whole call (upload, launches, copy back, synchronisation):
  freeze            DpgStore.freeze (grid, field and the copy into the map), wall time
  localize          dpg_fmap_localize against dpg_map_localize on one whole-map request at the library's
                    defaults: what the kept field saves
  track B           dpg_fmap_track at B = 1, 8, 64 and the default window (10 / 10 / 10 at 0.5 degrees),
                    guesses 3 cells and 1.5 degrees off the truth, against B calls of
                    dpg_fmap_localize(coarse_shift = 0) with the same window -- the only way to do this
                    without the tracker, the rebuild aside; the records must agree
  table bytes / s   the tracker's byte lookups of F per second (scans x angles x shifts x points / kernel
                    time) beside those dpg_fmap_localize calls: their bound phase, which at shift 0 scores
                    the whole volume (blocks x points, ms_bound; it also holds the key kernel and the seed
                    reduction), and their fine phase (frontier candidates x points, ms_fine)
Writes one JSON line per measurement to profiles/track/probe.jsonl.  Run on the GPU box:
    python tools/track_probe.py [--nodes-per-pass 2500 --beams 5000 --calls 10]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dpg-slam_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from dpgslam import _abi, api, synth  # noqa: E402
from dpgslam._abi import lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes-per-pass", type=int, default=2500)
    ap.add_argument("--beams", type=int, default=5000)
    ap.add_argument("--ratio", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track", "probe.jsonl"))
    a = ap.parse_args()

    t0 = time.time()
    w = synth.make_dynamic(n_passes=2, nodes_per_pass=a.nodes_per_pass, n_beams=a.beams, world_size=64.0, fov_deg=270.0,
                           n_boxes=48, range_noise=0.0)
    print(f"generated {w.V} nodes x {a.beams} beams in {time.time() - t0:.1f} s", flush=True)
    n0 = int(w.pass_start[1])
    ctx = api.Context(0)
    store = api.DpgStore(ctx, w.ranges[:n0], w.geom[:n0])
    est = np.ascontiguousarray(w.est[:n0])
    batches = [int(x) for x in a.batches.split(",")]
    n_scans = min(max(batches), w.V - n0)
    clouds = [np.ascontiguousarray(api.scan_to_cloud(w.ranges[n0 + k], w.geom[n0 + k, 0], w.geom[n0 + k, 1], w.geom[n0 + k, 2])[::a.ratio])
              for k in range(n_scans)]
    res = a.resolution
    guesses = [(float(w.est[n0 + k, 0]) + 3 * res, float(w.est[n0 + k, 1]) - 3 * res, float(w.est[n0 + k, 2]) + math.radians(1.5))
               for k in range(n_scans)]
    workload = {"nodes_in_map": n0, "beams": a.beams, "world_m": 64.0, "fov_deg": 270.0, "range_max_m": 30.0, "resolution": res,
                "scans": f"the first {n_scans} of pass 1, every {a.ratio}th point", "n_pts": int(len(clouds[0]))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").close()

    def emit(r):
        r["workload"] = workload
        print(json.dumps(r), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(r) + "\n")

    def timed(fn):
        """(median wall ms, the last result, every result) of a.calls calls after one uncounted."""
        fn()
        ts, out = [], []
        for _ in range(a.calls):
            t = time.perf_counter()
            out.append(fn())
            ts.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ts)), out[-1], out

    lp = _abi.default_loc_params()
    lp.resolution = res

    # freeze
    maps = []

    def freeze():
        maps.append(store.freeze(n0, est, lp))
        if len(maps) > 1:
            maps.pop(0).close()
        return maps[-1]
    ms, fmap, _ = timed(freeze)
    info = fmap.info()
    emit({"what": "freeze", "wall_ms": ms, "box": list(info["box"]), "field_bytes": info["n_bytes"], "calls": a.calls})

    # the global search, with and without the rebuild
    theta = float(w.est[n0, 2]) + math.radians(100.0)
    ms_s, _, rs = timed(lambda: store.localize(n0, est, clouds[0], (0.0, 0.0, theta), lp, window="map"))
    ms_m, _, rm = timed(lambda: fmap.localize(clouds[0], (0.0, 0.0, theta), lp, window="map"))
    assert all(all(x[n].tobytes() == rs[0][n].tobytes() for n in _abi.LOC_RESULT_EXACT) for x in rs + rm), "records differ"
    med = lambda xs, k: float(np.median([float(x[k]) for x in xs]))
    emit({"what": "localize", "window": "map", "coarse_shift": int(lp.coarse_shift), "calls": a.calls,
          "store": {"wall_ms": ms_s, "ms_kernels": med(rs, "ms_kernels"), "ms_field": med(rs, "ms_field")},
          "frozen": {"wall_ms": ms_m, "ms_kernels": med(rm, "ms_kernels"), "ms_field": med(rm, "ms_field")},
          "status": int(rm[0]["status"]), "n_blocks": int(rm[0]["n_blocks"]), "n_frontier": int(rm[0]["n_frontier"])})

    # the tracker against B single searches of the same window
    tp = _abi.default_track_params()
    sp = _abi.default_loc_params()
    sp.half_x, sp.half_y, sp.half_a, sp.angle_step = tp.half_x, tp.half_y, tp.half_a, tp.angle_step
    sp.coarse_shift, sp.max_refine_blocks = 0, 1 << 20
    volume = (2 * tp.half_a + 1) * (2 * tp.half_x + 1) * (2 * tp.half_y + 1)
    for B in batches:
        if B > n_scans:
            continue
        cl, gs = clouds[:B], guesses[:B]
        kms = []

        def track():
            r = fmap.track(cl, gs, tp)
            kms.append(float(lib().dpg_fmap_track_kernel_ms(fmap.handle)))
            return r
        ms_t, recs, allr = timed(track)
        assert all(x.tobytes() == recs.tobytes() for x in allr), "calls differ"
        ms_l, singles, _ = timed(lambda: [fmap.localize(c, g, sp) for c, g in zip(cl, gs)])
        assert all(all(np.array_equal(t[n], r[n]) for n in _abi.TRACK_RESULT_DTYPE.names) for t, r in zip(recs, singles)), "records differ"
        pts = sum(len(c) for c in cl)
        k_ms = float(np.median(kms[1:]))
        fine_ms = sum(float(r["ms_fine"]) for r in singles)
        cand = sum(int(r["n_refined_candidates"]) * int(r["n_pts"]) for r in singles)
        err = [math.hypot(float(r["pose"][0]) - float(w.est[n0 + k, 0]), float(r["pose"][1]) - float(w.est[n0 + k, 1])) for k, r in enumerate(recs)]
        emit({"what": "track", "B": B, "window": [int(tp.half_x), int(tp.half_y), int(tp.half_a)], "calls": a.calls, "points": pts,
              "track": {"wall_ms": ms_t, "kernel_ms": k_ms, "lookups": volume * pts, "lookups_per_s": volume * pts / (k_ms * 1e-3) if k_ms > 0 else None},
              "single_localize_calls": {"wall_ms": ms_l, "ms_kernels": sum(float(r["ms_kernels"]) for r in singles), "ms_fine": fine_ms,
                                        "ms_bound": sum(float(r["ms_bound"]) for r in singles),
                                        "bound_lookups": sum(int(r["n_blocks"]) * int(r["n_pts"]) for r in singles),
                                        "fine_lookups": cand, "fine_lookups_per_s": cand / (fine_ms * 1e-3) if fine_ms > 0 else None},
              "ok": int(sum(int(r["status"]) == _abi.DPG_LOC_OK for r in recs)), "worst_pose_error_m": max(err)})
    fmap.close()
    store.close()
    ctx.close()


if __name__ == "__main__":
    main()
