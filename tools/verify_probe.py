#!/usr/bin/env python3
"""Times the loop-closure verification (dpg_verify_batch) on config 4's loop-closure edges under their
own ICP transforms, at the default parameters, and reports how the default thresholds treat them.

One JSON line:
  verify_kernel_ms / verify_wall_ms   verify_kernel (HIP events around the launch) and the host wall
                      around the call, medians of --calls calls after one uncounted call
  points_per_s        moving points of both directions over kernel time
  csm_* / icp_*       the same edges through dpg_csm_batch and the batched ICP, as yardsticks
  lds_layout, lds_bytes, workgroups_per_cu_by_lds
                      the table layout and how many workgroups' LDS fit a CU's 160 KiB
  free_fraction, support_fraction     min / median / p90 / p99 / max over edges and directions of the
                      edges whose ICP converged
  rejected_by_defaults                how many of those api.verify_accept refuses at 0.15 / 0.25; config
                      4's estimates are near the truth, so this is the false-rejection count
  ref_equal           the first --ref-pairs records equal tests/verify_ref.py

  python tools/verify_probe.py [--calls 10] [--ref-pairs 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dpg-slam_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _dist(x):
    q = np.percentile(x, [0, 50, 90, 99, 100])
    return {k: round(float(v), 4) for k, v in zip(("min", "median", "p90", "p99", "max"), q)}


def _timed(fn, calls, kernel_ms):
    fn()   # uncounted
    wall, kern = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(kernel_ms())
    return out, float(np.median(kern)), float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--ref-pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls: at least 10")
    import verify_ref as V
    from dpgslam import _abi, api, synth
    w = synth.generate("config4")
    ip = _abi.default_icp_params()
    vp = _abi.default_verify_params()
    cp = _abi.default_csm_params()
    edges = np.ascontiguousarray(w.edges[w.n_successive:])
    with api.Context(0) as ctx:
        ctx.upload_scans(w.pts, w.offsets, ip.downsample_icp_points_ratio)
        (res, _), icp_ms, icp_wall = _timed(lambda: ctx.icp_batch(edges, w.est, ip, compute_cov=False), a.calls, ctx.icp_kernel_ms)
        T = np.ascontiguousarray(res["T"])
        rec, ver_ms, ver_wall = _timed(lambda: ctx.verify_batch(edges, T, vp), a.calls, ctx.verify_kernel_ms)
        _, csm_ms, csm_wall = _timed(lambda: ctx.csm_batch(edges, poses=w.est, params=cp), a.calls, ctx.csm_kernel_ms)
    ds = {}
    for k in range(a.ref_pairs):
        t, s = (int(v) for v in edges[k])
        for v in (t, s):
            if v not in ds:
                ds[v] = api.downsample(w.cloud(v), ip.downsample_icp_points_ratio)
        assert rec[k].tobytes() == V.result(ds[t], ds[s], T[k], vp).tobytes(), "the kernel's record differs from the reference"
    conv = (res["converged"] != 0) & (res["status"] == _abi.DPG_ICP_OK)
    r = rec[conv]
    den = np.maximum(r["n_in"], 1)
    lds = api.verify_lds_bytes(vp)
    line = json.dumps({
        "what": "verify_batch", "workload": "config4 loop closures", "edges": int(len(edges)), "converged": int(conv.sum()),
        "moving_points": int(rec["n_pts"].sum()), "params": {"resolution": vp.resolution, "half_cells": vp.half_cells,
                                                             "occ_radius": vp.occ_radius, "sensor": [vp.sensor[0], vp.sensor[1]]},
        "calls": a.calls, "verify_kernel_ms": round(ver_ms, 4), "verify_wall_ms": round(ver_wall, 4),
        "points_per_s": round(float(rec["n_pts"].sum()) / (ver_ms * 1e-3), 1),
        "csm_kernel_ms": round(csm_ms, 4), "csm_wall_ms": round(csm_wall, 4),
        "icp_kernel_ms": round(icp_ms, 4), "icp_wall_ms": round(icp_wall, 4),
        "lds_layout": "two bit planes, LDS atomicOr", "lds_bytes": lds, "workgroups_per_cu_by_lds": int(160 * 1024 // lds),
        "status_no_overlap": int((r["status"] != _abi.DPG_VERIFY_OK).sum()),
        "free_fraction": _dist((r["n_free"] / den).ravel()), "support_fraction": _dist((r["n_support"] / den).ravel()),
        "rejected_by_defaults": int((~api.verify_accept(r)).sum()), "thresholds": [0.15, 0.25],
        "ref_pairs": a.ref_pairs, "ref_equal": True})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
