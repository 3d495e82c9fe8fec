"""The joint-marginal interface without a GPU: the header's declarations, the ctypes bindings, the
Python wrappers' argument checks (before any call into the library), and the host planner
(dpg_chol_plan_joint_pairs / _nodes) against brute force in a stand-alone program built with the
address and undefined-behaviour sanitizers (tools/joint_plan_check.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_marginals_cpu import _NoLib, _bare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAIRS = r"\(\s*{h}\s*{a},\s*const int32_t\*\s*pairs[^,]*,\s*int64_t\s+n,\s*double\*\s*cov_out"
NODES = r"\(\s*{h}\s*{a},\s*const int32_t\*\s*nodes,\s*int64_t\s+n,\s*double\*\s*cov_out"
DECLS = {
    "dpg_gn_cross_covariances": PAIRS.format(h=r"dpg_ctx\*", a="ctx"),
    "dpg_gn_joint_marginal": NODES.format(h=r"dpg_ctx\*", a="ctx"),
    "dpg_gn_relative_covariances": PAIRS.format(h=r"dpg_ctx\*", a="ctx"),
    "dpg_inc_cross_covariances": PAIRS.format(h=r"dpg_inc\*", a="g"),
    "dpg_inc_joint_marginal": NODES.format(h=r"dpg_inc\*", a="g"),
    "dpg_inc_relative_covariances": PAIRS.format(h=r"dpg_inc\*", a="g"),
}


def test_header_declares_the_six_functions():
    with open(os.path.join(ROOT, "include", "dpg_slam_c.h")) as f:
        h = f.read()
    for name, args in DECLS.items():
        assert re.search(r"int\s+" + name + args, h), name
    for word in ("jointmarginalcovariance", "solve_inv_cols", "-ad(z^-1)", "zero matrix for i == j"):
        assert word in h.lower(), word


def test_abi_binds_them_with_the_declared_types():
    from dpgslam import _abi
    P, I32P, F64P, I64 = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int64
    L = _abi.lib()
    for name in DECLS:
        fn = getattr(L, name)
        assert fn.restype is C.c_int, name
        assert list(fn.argtypes) == [P, I32P, I64, F64P], name
        assert _abi.SIGNATURES[name] == (C.c_int, [P, I32P, I64, F64P]), name


@pytest.fixture
def no_lib(monkeypatch):
    from dpgslam import api
    monkeypatch.setattr(api, "lib", lambda: _NoLib())
    return api


@pytest.mark.parametrize("pairs", [[0, 1], [[0, 1, 2]], [[0.0, 1.0]], np.zeros((2, 2, 2), np.int32)])
def test_wrappers_reject_malformed_pairs(no_lib, pairs):
    api = no_lib
    ctx = _bare(api.Context, handle=None)
    inc = _bare(api.IncGraph, handle=None)
    for fn in (ctx.gn_cross_covariances, ctx.gn_relative_covariances, inc.cross_covariances, inc.relative_covariances):
        with pytest.raises(ValueError, match="pairs"):
            fn(pairs)


@pytest.mark.parametrize("nodes", [[[0, 1], [2, 3]], 3, [0.5, 1.0], np.zeros((2, 1), np.int32), None])
def test_wrappers_reject_malformed_nodes(no_lib, nodes):
    api = no_lib
    ctx = _bare(api.Context, handle=None)
    inc = _bare(api.IncGraph, handle=None)
    for fn in (ctx.gn_joint_marginal, inc.joint_marginal):
        with pytest.raises(ValueError, match="nodes"):
            fn(nodes)


def test_get_relative_pose_covariance_needs_a_backend_method():
    """A backend without `relative_covariances` gets an error naming the method; GpuBackend has it."""
    from dpgslam.slam import DpgSLAM, GpuBackend
    from slam_oracle import OracleSlamBackend
    assert callable(getattr(GpuBackend, "relative_covariances"))
    s = DpgSLAM(backend=OracleSlamBackend())
    with pytest.raises(ValueError):
        s.GetRelativePoseCovariance(0, 0)      # no node yet
    s.poses = np.zeros((2, 3), np.float32)
    with pytest.raises(NotImplementedError, match="relative_covariances"):
        s.GetRelativePoseCovariance(0, 1)
    with pytest.raises(IndexError):
        s.GetRelativePoseCovariance(0, 2)
    with pytest.raises(IndexError):
        s.GetRelativePoseCovariance(-1, 1)


def test_planner_against_brute_force_under_sanitizers(tmp_path):
    """Every query's path, length and first row, every block's common-suffix length and slice
    offsets, W slices without overlap and inside the reported size, every output element written
    once -- on a chain, a mesh, a forest and a band graph under md, nd and the automatic order."""
    exe = str(tmp_path / "joint_plan_check")
    csrc = os.path.join(ROOT, "dpg-slam_amd", "csrc")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-pthread", "-o", exe,
                        os.path.join(ROOT, "tools", "joint_plan_check.cpp"), os.path.join(csrc, "dpg_chol_sym.cpp"),
                        os.path.join(csrc, "dpg_chol_plan.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "joint plan check ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    # the band graph reaches the path solve's global-memory route under the default order
    assert re.search(r"band n=130 order=0 cols=64 .*global memory", r.stdout)
