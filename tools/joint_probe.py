#!/usr/bin/env python3
"""Times the joint marginals of random node pairs (dpg_gn_cross_covariances) on configs 2, 3 and 4
with their ICP factors, at the poses optimize_graph reaches (the set-up of tools/marginals_probe.py).

One JSON line per config:
  cross_ms            per pair count (1, 64, 4096 random pairs): wall ms of one
                      dpg_gn_cross_covariances call (re-linearization, factorization, plan, path
                      solve, dot, copy out), median of --calls calls after --warmup
  path_ms, dot_ms     the two kernels of the same requests (HIP events), medians
  path_fronts,        the longest root path of the analysis, in fronts and in pivot scalars
  path_scalars
  marginals_ms        dpg_gn_marginals of all nodes, and
  factor_ms           one factorization (+ its triangular solves), from gn_marginals_profile: the
                      yardsticks of profiles/marginals

  python tools/joint_probe.py [--configs config2,config3,config4] [--calls 10] [--warmup 2] [--out FILE]
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

COUNTS = (1, 64, 4096)


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
    rng = np.random.default_rng(1)
    out = {"config": name, "V": int(w.V), "factors": int(len(F)), "calls": calls, "warmup": warmup}
    for n in COUNTS:
        pairs = rng.integers(0, w.V, (n, 2)).astype(np.int32)
        wall, prof = [], []
        for k in range(warmup + calls):
            t = time.perf_counter()
            S = ctx.gn_cross_covariances(pairs)
            dt = (time.perf_counter() - t) * 1e3
            pr = ctx.gn_joint_profile(pairs)
            if k >= warmup:
                wall.append(dt)
                prof.append(pr)
        assert np.all(np.isfinite(S))
        out[f"cross_ms_{n}"] = round(float(np.median(wall)), 4)
        out[f"path_ms_{n}"] = round(float(np.median([q["path_ms"] for q in prof])), 4)
        out[f"dot_ms_{n}"] = round(float(np.median([q["dot_ms"] for q in prof])), 4)
        out[f"distinct_nodes_{n}"] = int(len(np.unique(pairs)))
        out["path_fronts"], out["path_scalars"] = prof[0]["path_fronts"], prof[0]["path_scalars"]
    wall, prof = [], []
    for k in range(warmup + calls):
        t = time.perf_counter()
        ctx.gn_marginals()
        dt = (time.perf_counter() - t) * 1e3
        pr = ctx.gn_marginals_profile()
        if k >= warmup:
            wall.append(dt)
            prof.append(pr)
    out["marginals_ms"] = round(float(np.median(wall)), 4)
    out["factor_ms"] = round(float(np.median([q["factor_ms"] for q in prof])), 4)
    return out


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
