"""Occupancy-grid probe: dpg_occupancy_grid on the node store of the `--workload dpg`
benchmark (config 5: 4 passes x 2500 nodes of a 64 m building, 5000-beam 270-degree 30 m scans, 48
movable boxes, ground-truth poses), every node active -- the largest grid that store can ask for.

Per resolution (0.05, 0.10) and per raster-kernel variant (dpg_grid_params.pad: lane group /
workgroup / LDS table slots; 0 is the product) the median of --calls calls: the HIP-event kernel
time, n_samples, samples/s, and the global atomics per sample (flushed LDS slots + direct adds).
Every variant's grid must equal variant 0's.  The yardstick beside it is the existing bit-setting
rasteriser on the same store: n_samples / ms_kernels of dpg_execute_dpg calls that rebuild their
window (dpg_dpg_load invalidates it before each call), median over the same number of calls.
Writes one JSON line per measurement to profiles/occupancy_grid/probe.jsonl.  Run on the GPU box:
    python tools/occ_grid_probe.py [--nodes-per-pass 2500 --beams 5000 --calls 10]
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dpg-slam_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from dpgslam import _abi, api, synth  # noqa: E402

VARIANTS = {0: (8, 1024, 8192), 1: (32, 1024, 8192), 2: (16, 1024, 8192), 3: (8, 1024, 8192), 4: (4, 1024, 8192),
            5: (8, 512, 4096), 6: (16, 512, 4096), 7: (32, 1024, 0), 8: (8, 512, 8192), 9: (4, 512, 4096)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--nodes-per-pass", type=int, default=2500)
    ap.add_argument("--beams", type=int, default=5000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--variants", default="0,1,2,3,4,5,6,7,8,9")
    ap.add_argument("--resolutions", default="0.05,0.10")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occupancy_grid", "probe.jsonl"))
    a = ap.parse_args()

    t0 = time.time()
    w = synth.make_dynamic(n_passes=a.passes, nodes_per_pass=a.nodes_per_pass, n_beams=a.beams, world_size=64.0,
                           fov_deg=270.0, n_boxes=48, range_noise=0.0)
    gen_s = time.time() - t0
    print(f"generated {w.V} nodes x {a.beams} beams in {gen_s:.1f} s", flush=True)
    ctx = api.Context(0)
    g = api.DpgStore(ctx, w.ranges, w.geom)
    workload = {"passes": a.passes, "nodes_per_pass": a.nodes_per_pass, "beams": a.beams, "nodes": int(w.V),
                "world_m": 64.0, "fov_deg": 270.0, "range_max_m": 30.0, "state": "every node and sector active"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").close()

    def emit(r):
        print(json.dumps(r), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(r) + "\n")

    for res in [float(x) for x in a.resolutions.split(",")]:
        want = None
        for v in [int(x) for x in a.variants.split(",")]:
            p = _abi.default_grid_params()
            p.resolution = res
            p.pad = v
            ms, tot, calls = [], [], a.calls
            k = 0
            while k < calls + 1:                  # the first call (allocation, cold caches) is not counted
                out = g.occupancy_grid(w.V, w.est, p, counts=True)
                if k:
                    ms.append(out["info"].ms_kernels)
                    tot.append(out["info"].ms_total)
                elif out["info"].ms_kernels > 2000.0:
                    calls = min(calls, 3)         # a variant this slow is not in the running: three calls place it
                k += 1
            info = out["info"]
            h = hashlib.sha256(out["hits"].tobytes() + out["misses"].tobytes() + out["data"].tobytes()).hexdigest()
            if want is None:
                want = h
            m = float(np.median(ms))
            G, RB, H = VARIANTS[v]
            emit({"what": "occupancy_grid", "resolution": res, "variant": v, "lane_group": G, "block": RB, "lds_slots": H,
                  "lds_bytes": 8 * H, "calls": calls, "ms_kernels_median": m, "ms_kernels_min": float(min(ms)),
                  "ms_total_median": float(np.median(tot)), "width": int(info.w), "height": int(info.h),
                  "n_nodes_used": int(info.n_nodes_used), "n_beams_used": int(info.n_beams_used),
                  "n_hits": int(info.n_hits), "n_samples": int(info.n_samples), "n_oob": int(info.n_oob),
                  "n_direct": int(info.n_direct), "n_flushed": int(info.n_flushed),
                  "samples_per_s": info.n_samples / (m * 1e-3),
                  "global_atomics_per_sample": (info.n_direct + info.n_flushed) / max(int(info.n_samples), 1),
                  "equals_variant_0": h == want, "workload": workload})
            assert h == want, f"variant {v} differs from variant 0 at resolution {res}"

    # yardstick: the bit-setting rasteriser (raster_kernel, 32 / 1024 / 16 K slots) inside executeDPG calls that
    # rebuild their window, on the same store; ms_kernels covers the whole call's device work
    n0 = int(w.pass_start[1])
    picks = np.linspace(n0, w.V - 1, a.calls + 1).astype(int)
    rate, recs = [], []
    for k, v in enumerate(picks):
        g.load()                                   # invalidates the kept window: the call rebuilds it
        st = g.execute_dpg(int(v) + 1, int(v - w.pass_start[w.pass_of[v]] + 1), w.est[:v + 1])
        if k:
            rate.append(st.n_samples / (st.ms_kernels * 1e-3))
            recs.append({"node": int(v), "n_samples": int(st.n_samples), "ms_kernels": float(st.ms_kernels),
                         "n_candidates": int(st.n_candidates), "grid_cells": int(st.grid_cells)})
    emit({"what": "yardstick_execute_dpg_rebuild", "resolution": float(g.params.occ_grid_resolution), "calls": a.calls,
          "samples_per_s_median": float(np.median(rate)), "samples_per_s_min": float(min(rate)),
          "samples_per_s_max": float(max(rate)), "per_call": recs, "workload": workload,
          "note": "n_samples / ms_kernels of dpg_execute_dpg (all its kernels: window reset, three raster passes, "
                  "histogram, detection, labels, sector update), window rebuilt by every call"})
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
