"""Localisation probe: dpg_map_localize on the node store of the `--workload dpg`
benchmark (config 5: passes of 2500 nodes of a 64 m building, 5000-beam 270-degree 30 m scans, 48
movable boxes, ground-truth poses).  The map is pass 0 with every node active; the scan is the first
of pass 1, every --ratio-th point of it.

Per resolution (0.05, 0.10) and coarse_shift (0 .. 5), the full circle at 0.5 degrees:
  window "map"    the whole box (DpgStore.localize(window="map")), the guess's angle 100 degrees off;
  window "local"  +-128 cells around a guess 4 cells and 100 degrees off the truth, where the
                  exhaustive search (coarse_shift 0) fits the bound volume: what the pruning buys.
Each setting: one uncounted call, then the median of --calls calls of the HIP-event times (field
build, bound phase, fine phase), the frontier's size, the candidates refined, and the bound phase's
table-byte lookups per second (blocks x points / bound time; the phase also holds the key kernel and
the per-angle seed reduction).  A frontier above --max-refine-blocks (4096 unless given) is measured a
second time with room for it.  A setting the call refuses (DPG_ERR_SIZE: a bound volume above 2^29 blocks) is
recorded as refused, not measured.  Every proven result of one window must name the same candidate.
Writes one JSON line per measurement to profiles/localize/probe.jsonl.  Run on the GPU box:
    python tools/loc_probe.py [--nodes-per-pass 2500 --beams 5000 --calls 10]
The library's defaults alone (profiles/localize/defaults.jsonl):
    python tools/loc_probe.py --shifts 4 --max-refine-blocks 16384 --out profiles/localize/defaults.jsonl
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

CSM_LOOKUPS_PER_S = 9.0e12   # DESIGN K9: the pair matcher's lane lookups per second, its table in LDS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes-per-pass", type=int, default=2500)
    ap.add_argument("--beams", type=int, default=5000)
    ap.add_argument("--ratio", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--resolutions", default="0.05,0.10")
    ap.add_argument("--shifts", default="0,1,2,3,4,5")
    ap.add_argument("--max-refine-blocks", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize", "probe.jsonl"))
    a = ap.parse_args()

    t0 = time.time()
    w = synth.make_dynamic(n_passes=2, nodes_per_pass=a.nodes_per_pass, n_beams=a.beams, world_size=64.0, fov_deg=270.0,
                           n_boxes=48, range_noise=0.0)
    print(f"generated {w.V} nodes x {a.beams} beams in {time.time() - t0:.1f} s", flush=True)
    n0 = int(w.pass_start[1])
    ctx = api.Context(0)
    store = api.DpgStore(ctx, w.ranges[:n0], w.geom[:n0])
    est = np.ascontiguousarray(w.est[:n0])
    truth = w.est[n0].astype(np.float64)
    cloud = np.ascontiguousarray(api.scan_to_cloud(w.ranges[n0], w.geom[n0, 0], w.geom[n0, 1], w.geom[n0, 2])[::a.ratio])
    workload = {"nodes_in_map": n0, "beams": a.beams, "world_m": 64.0, "fov_deg": 270.0, "range_max_m": 30.0,
                "scan": f"first of pass 1, every {a.ratio}th point", "n_pts": int(len(cloud)), "truth": truth.tolist()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").close()

    def emit(r):
        print(json.dumps(r), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(r) + "\n")

    def measure(res, shift, window, cap):
        p = _abi.default_loc_params()
        p.resolution, p.coarse_shift, p.max_refine_blocks = res, shift, cap
        theta = truth[2] + math.radians(100.0)
        if window == "map":
            guess, kw = (0.0, 0.0, theta), dict(window="map")
        else:
            p.half_x = p.half_y = 128
            guess, kw = (truth[0] + 4 * res, truth[1] - 4 * res, theta), {}
        rec = {"what": "localize", "resolution": res, "coarse_shift": shift, "window": window, "max_refine_blocks": cap,
               "half_a": int(p.half_a), "angle_step_deg": 0.5, "calls": a.calls}
        rs = []
        try:
            for k in range(a.calls + 1):           # the first call (allocation, cold caches) is not counted
                r = store.localize(n0, est, cloud, guess, p, **kw)
                if k:
                    rs.append(r)
                elif float(r["ms_kernels"]) > 500.0:
                    rec["calls"] = 3               # a setting this slow: three calls place it
                if len(rs) >= rec["calls"]:
                    break
        except _abi.DpgError as e:
            rec.update(refused=str(e))
            return rec, None
        r = rs[-1]
        assert all(all(x[n].tobytes() == r[n].tobytes() for n in _abi.LOC_RESULT_EXACT) for x in rs), "calls differ"
        med = {k: float(np.median([float(x[k]) for x in rs])) for k in ("ms_field", "ms_bound", "ms_fine", "ms_kernels")}
        lookups = int(r["n_blocks"]) * int(r["n_pts"])
        pose = r["pose"].astype(np.float64)
        rec.update(med, box=[int(b) for b in r["box"]], n_pts=int(r["n_pts"]), n_blocks=int(r["n_blocks"]),
                   n_frontier=int(r["n_frontier"]), n_refined_candidates=int(r["n_refined_candidates"]),
                   status=int(r["status"]), score=int(r["score"]), response=int(r["score"]) / (255.0 * max(int(r["n_pts"]), 1)),
                   winner=[int(r["best_a"]), int(r["best_dx"]), int(r["best_dy"])], pose=pose.tolist(),
                   pose_error_m=math.hypot(pose[0] - truth[0], pose[1] - truth[1]),
                   pose_error_deg=abs(math.degrees(math.remainder(pose[2] - truth[2], 2 * math.pi))),
                   bound_lookups=lookups, bound_lookups_per_s=lookups / (med["ms_bound"] * 1e-3) if med["ms_bound"] > 0 else None,
                   csm_lane_lookups_per_s=CSM_LOOKUPS_PER_S)
        return rec, r

    for res in [float(x) for x in a.resolutions.split(",")]:
        for window in ("map", "local"):
            proven = {}
            for shift in [int(x) for x in a.shifts.split(",")]:
                rec, r = measure(res, shift, window, a.max_refine_blocks)
                rec["workload"] = workload
                emit(rec)
                if r is not None and int(r["status"]) == _abi.DPG_LOC_UNPROVEN and int(r["n_frontier"]) <= 1 << 24:
                    rec, r = measure(res, shift, window, int(r["n_frontier"]))
                    rec["workload"] = workload
                    emit(rec)
                if r is not None and int(r["status"]) == _abi.DPG_LOC_OK:
                    proven[shift] = (rec["winner"], rec["pose"], rec["score"])
            assert len({json.dumps(v) for v in proven.values()}) <= 1, f"proven results differ: {proven}"
    store.close()
    ctx.close()


if __name__ == "__main__":
    main()
