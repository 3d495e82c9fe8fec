"""Field-refinement probe, on the frozen map of tools/track_probe.py (config 5: pass 0
of 2500 nodes of a 64 m building, 5000-beam 270-degree 30 m scans, 48 movable boxes, ground-truth
poses; frozen at 0.05 m).  The scans are the first of pass 1, every --ratio-th point of each (1000
points), tracked from guesses 3 cells and 1.5 degrees off the truth in the default window.

Each figure: one uncounted call, then the median of --calls calls.
  track B / track_refine B   dpg_fmap_track and dpg_fmap_track_refine at B = 1, 8, 64: the HIP-event
                    time of the tracker's two launches and of the refinement launch, and the wall time
                    of the whole call (upload, launches, copy back, synchronisation)
  icp per scan      the only refinement there was before: DpgSLAM.StartLocalization(icp_refine=True)'s
                    step, one run_icp per scan from the tracked pose against the nearest node's stored
                    cloud, at the library's ICP defaults; wall ms per scan, from Python as that mode runs it
  errors            the distance from the ground truth of the raw track pose, of the field-refined pose
                    and of the ICP-refined pose (median and worst over the batch), the evaluations per
                    scan and the statuses
Writes one JSON line per measurement to profiles/refine/probe.jsonl.  Run on the GPU box:
    python tools/refine_probe.py [--nodes-per-pass 2500 --beams 5000 --calls 10]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes-per-pass", type=int, default=2500)
    ap.add_argument("--beams", type=int, default=5000)
    ap.add_argument("--ratio", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine", "probe.jsonl"))
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
    truth = [tuple(float(v) for v in w.est[n0 + k]) for k in range(n_scans)]
    guesses = [(t[0] + 3 * res, t[1] - 3 * res, t[2] + math.radians(1.5)) for t in truth]
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
        """(median wall ms, the last result) of a.calls calls after one uncounted."""
        fn()
        ts, out = [], None
        for _ in range(a.calls):
            t = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ts)), out

    def errs(poses):
        d = [math.hypot(float(p[0]) - t[0], float(p[1]) - t[1]) for p, t in zip(poses, truth)]
        ang = [abs(math.remainder(float(p[2]) - t[2], 2 * math.pi)) for p, t in zip(poses, truth)]
        return {"median_m": float(np.median(d)), "worst_m": float(max(d)), "median_deg": math.degrees(float(np.median(ang))),
                "worst_deg": math.degrees(float(max(ang)))}

    lp = _abi.default_loc_params()
    lp.resolution = res
    fmap = store.freeze(n0, est, lp)
    tp, rp, ip = _abi.default_track_params(), _abi.default_refine_params(), _abi.default_icp_params()
    node_clouds = {}

    def node_cloud(t):
        if t not in node_clouds:
            node_clouds[t] = api.scan_to_cloud(w.ranges[t], w.geom[t, 0], w.geom[t, 1], w.geom[t, 2])
        return node_clouds[t]

    for B in batches:
        if B > n_scans:
            continue
        cl, gs = clouds[:B], guesses[:B]
        k_track, k_fused_t, k_fused_r = [], [], []

        def track():
            r = fmap.track(cl, gs, tp)
            k_track.append(fmap.track_kernel_ms())
            return r

        def fused():
            r = fmap.track_refine(cl, gs, tp, rp)
            k_fused_t.append(fmap.track_kernel_ms())
            k_fused_r.append(fmap.refine_kernel_ms())
            return r
        ms_t, trecs = timed(track)
        ms_f, (t2, frecs) = timed(fused)
        assert t2.tobytes() == trecs.tobytes(), "the fused call's track records differ"
        assert frecs.tobytes() == fmap.refine(cl, trecs, rp).tobytes(), "the fused call's refine records differ"

        # the ICP step of StartLocalization(icp_refine=True), scan by scan
        def icp_all():
            out = []
            for c, r in zip(cl, trecs):
                pose = np.array(r["pose"], np.float32)
                d = est[:, :2].astype(np.float64) - pose[:2].astype(np.float64)
                t = int(np.argmin(d[:, 0] ** 2 + d[:, 1] ** 2))
                ok, z, *_ = ctx.run_icp(api.Node(est[t], node_cloud(t)), api.Node(pose, c), ip)
                out.append((bool(ok), api.transform_point(np.array([z[0][0], z[0][1], z[1]], np.float32), est[t]) if ok else pose))
            return out
        ms_i, icp = timed(icp_all)
        emit({"what": "track_refine", "B": B, "calls": a.calls, "points": int(sum(len(c) for c in cl)),
              "window": [int(tp.half_x), int(tp.half_y), int(tp.half_a)], "max_iters": int(rp.max_iters),
              "track": {"wall_ms": ms_t, "kernel_ms": float(np.median(k_track[1:]))},
              "track_refine": {"wall_ms": ms_f, "track_kernel_ms": float(np.median(k_fused_t[1:])),
                               "refine_kernel_ms": float(np.median(k_fused_r[1:]))},
              "icp_per_scan": {"wall_ms_per_scan": ms_i / B, "converged": int(sum(ok for ok, _ in icp))},
              "error_track": errs([r["pose"] for r in trecs]), "error_field_refine": errs([r["pose"] for r in frecs]),
              "error_icp_refine": errs([p for _, p in icp]),
              "evaluations": {"median": float(np.median(frecs["n_evals"])), "max": int(frecs["n_evals"].max()),
                              "best_eval_median": float(np.median(frecs["best_eval"]))},
              "status_counts": [int((frecs["status"] == s).sum()) for s in range(4)],
              "cov_ok": int(frecs["cov_ok"].sum()), "track_ok": int((trecs["status"] == _abi.DPG_LOC_OK).sum())})
    fmap.close()
    store.close()
    ctx.close()


if __name__ == "__main__":
    main()
