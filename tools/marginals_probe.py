#!/usr/bin/env python3
"""Times the marginal covariances of all nodes (dpg_gn_marginals) on configs 2, 3 and 4 with their
ICP factors (as tests/test_gpu_solver.py builds them), at the poses optimize_graph reaches.

One JSON line per config:
  marginals_ms        wall ms of one dpg_gn_marginals call for all nodes (re-linearization,
                      factorization, selected inversion, gather, copy out): median of --calls calls
                      after --warmup
  selinv_ms           sum of the selected inversion's launches (HIP events), median over the calls
  level_ms            the launches one by one, the roots' level first (median per level)
  factor_ms           the factorization (+ its triangular solves) of the same calls, HIP events
  selinv_over_factor  selinv_ms / factor_ms
  sigma_bytes         the Sigma buffer and the large fronts' work buffer

  python tools/marginals_probe.py [--configs config2,config3,config4] [--calls 10] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dpg-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def probe(ctx, name, calls, warmup):
    from dpgslam import _abi, synth
    w = synth.generate(name)
    p = _abi.default_icp_params()
    ctx.upload_scans(w.pts, w.offsets, 5)
    res, _ = ctx.icp_batch(w.edges, w.est, p, compute_cov=False)
    F = w.factors_with_icp(res, p)
    X, st = ctx.optimize_graph(w.est.astype(np.float64), F)
    ctx.gn_setup(w.V, F)
    ctx.gn_set_poses(X)
    wall, prof = [], []
    for k in range(warmup + calls):
        t = time.perf_counter()
        S = ctx.gn_marginals()
        dt = (time.perf_counter() - t) * 1e3
        pr = ctx.gn_marginals_profile()
        if k >= warmup:
            wall.append(dt)
            prof.append(pr)
    lv = np.median(np.array([q["level_ms"] for q in prof]), axis=0)
    sel = float(np.median([sum(q["level_ms"]) for q in prof]))
    fac = float(np.median([q["factor_ms"] for q in prof]))
    return {"config": name, "V": int(w.V), "factors": int(len(F)), "calls": calls, "warmup": warmup,
            "marginals_ms": round(float(np.median(wall)), 4), "marginals_ms_min": round(float(np.min(wall)), 4),
            "selinv_ms": round(sel, 4), "factor_ms": round(fac, 4),
            "assemble_ms": round(float(np.median([q["assemble_ms"] for q in prof])), 4),
            "selinv_over_factor": round(sel / fac, 3), "levels": prof[0]["levels"],
            "level_ms": [round(float(x), 4) for x in lv], "sigma_bytes": prof[0]["sigma_bytes"],
            "max_sigma_trace": float(np.trace(S, axis1=1, axis2=2).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="config2,config3,config4")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls: at least 10")
    from dpgslam import api
    lines = []
    with api.Context(0) as ctx:
        for name in a.configs.split(","):
            line = json.dumps(probe(ctx, name, a.calls, a.warmup))
            print(line, flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
