"""bench.py's command line: a plain run (set-up, warm-up, the timed steps, the result line), --full
(the CPU baselines, the cold single solve and the caller's-order ICP runs beside it) and
--dump-outputs DIR (what the last timed step computed, one float .npy per array)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("icp_T", "icp_z", "icp_flags", "icp_fitness", "icp_cov_hessian", "gn_poses", "gn_stats")


def test_dump_outputs_writes_float_arrays(tmp_path):
    import bench
    from dpgslam import _abi

    rng = np.random.default_rng(0)
    n, V = 7, 5
    res = np.zeros(n, _abi.RESULT_DTYPE)
    res["T"] = rng.standard_normal((n, 6)).astype(np.float32)
    res["z"] = rng.standard_normal((n, 3)).astype(np.float32)
    res["converged"], res["iterations"], res["n_corr"], res["status"] = 1, np.arange(n), 100 + np.arange(n), 0
    res["fitness"] = rng.random(n)
    hess = rng.standard_normal((n, 3, 3))
    X = rng.standard_normal((V, 3))
    out = str(tmp_path / "dump")
    bench.dump_outputs(out, res, hess, X, {"iterations": 8, "final_error": 0.25})
    assert sorted(os.listdir(out)) == sorted(name + ".npy" for name in NAMES)
    got = {name: np.load(os.path.join(out, name + ".npy")) for name in NAMES}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["icp_T"], res["T"]) and np.array_equal(got["icp_z"], res["z"])
    assert np.array_equal(got["icp_flags"][:, 1], np.arange(n)) and np.array_equal(got["icp_flags"][:, 2], 100 + np.arange(n))
    assert np.array_equal(got["icp_fitness"], res["fitness"]) and np.array_equal(got["icp_cov_hessian"], hess)
    assert np.array_equal(got["gn_poses"], X) and got["gn_stats"].tolist() == [8.0, 0.25]


def test_help_names_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path, ctx, workload):
    """One plain run on config 2: the line has the headline's fields and none of --full's legs,
    --steps sets the timed steps, and the dumped ICP results are the ones the same batch gives
    in-process (the ICP path is bit-exact)."""
    from dpgslam import _abi

    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--config", "config2", "--dump-outputs", out], capture_output=True, text=True, timeout=120,
                       env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["unit"] == "edges/s"
    assert line["cpu_baseline"] is None and "cold_single_solve" not in line and "icp_kernel_ms_caller_order" not in line
    w = workload("config2")
    got = {name: np.load(os.path.join(out, name + ".npy")) for name in NAMES}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["icp_z"].shape == (w.E, 3) and got["icp_cov_hessian"].shape == (w.E, 3, 3) and got["gn_poses"].shape == (w.V, 3)
    ctx.upload_scans(w.pts, w.offsets, _abi.default_icp_params().downsample_icp_points_ratio)
    res, hess = ctx.icp_batch(w.edges, w.est, _abi.default_icp_params())
    assert np.array_equal(got["icp_T"], res["T"]) and np.array_equal(got["icp_z"], res["z"])
    assert np.array_equal(got["icp_flags"][:, 1], res["iterations"])
    np.testing.assert_allclose(got["icp_cov_hessian"], hess, rtol=1e-12, atol=1e-8)   # test_gpu_parity's bound
    assert np.isfinite(got["gn_poses"]).all() and got["gn_stats"][0] == line["gn_iterations"]
    assert got["gn_stats"][1] == line["final_error"]
