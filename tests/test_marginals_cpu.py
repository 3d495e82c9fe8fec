"""The marginals interface without a GPU: the header's declarations, the ctypes bindings, and the
Python wrappers' argument checks (which come before any call into the library)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "dpg_gn_marginals": r"int\s+dpg_gn_marginals\(\s*dpg_ctx\*\s*ctx,\s*const int32_t\*\s*nodes,\s*int64_t\s+n,\s*double\*\s*cov_out",
    "dpg_gn_marginal_pairs": r"int\s+dpg_gn_marginal_pairs\(\s*dpg_ctx\*\s*ctx,\s*const int32_t\*\s*pairs[^,]*,\s*int64_t\s+n,\s*double\*\s*cov_out",
    "dpg_marginal_covariances": r"int\s+dpg_marginal_covariances\(\s*dpg_ctx\*\s*ctx,\s*const double\*\s*poses,\s*int64_t\s+n_nodes,"
                                r"\s*const dpg_factor\*\s*factors,\s*int64_t\s+n_factors,\s*const int32_t\*\s*nodes,\s*int64_t\s+n,"
                                r"\s*double\*\s*cov_out\)",
    "dpg_inc_marginals": r"int\s+dpg_inc_marginals\(\s*dpg_inc\*\s*g,\s*const int32_t\*\s*nodes,\s*int64_t\s+n,\s*double\*\s*cov_out",
}


def test_header_declares_the_four_functions():
    with open(os.path.join(ROOT, "include", "dpg_slam_c.h")) as f:
        h = f.read()
    for name, pat in DECLS.items():
        assert re.search(pat, h), name
    # the conventions the header must state
    for word in ("tangent", "dpg_solver_pcg", "theta", "duplicate_factors", "more than one rank"):
        assert word in h.lower(), word


def test_abi_binds_them_with_the_declared_types():
    from dpgslam import _abi
    P, I32P, F64P, I64 = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int64
    want = {
        "dpg_gn_marginals": (C.c_int, [P, I32P, I64, F64P]),
        "dpg_gn_marginal_pairs": (C.c_int, [P, I32P, I64, F64P]),
        "dpg_marginal_covariances": (C.c_int, [P, F64P, I64, P, I64, I32P, I64, F64P]),
        "dpg_inc_marginals": (C.c_int, [P, I32P, I64, F64P]),
    }
    L = _abi.lib()
    for name, (res, args) in want.items():
        fn = getattr(L, name)
        assert fn.restype is res, name
        assert list(fn.argtypes) == args, name


class _NoLib:
    """Stands in for the library: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called into the library ({name}) before checking its arguments")


@pytest.fixture
def no_lib(monkeypatch):
    from dpgslam import api
    monkeypatch.setattr(api, "lib", lambda: _NoLib())
    return api


def _bare(cls, **attrs):
    o = cls.__new__(cls)
    o.__dict__.update(attrs)
    return o


@pytest.mark.parametrize("nodes", [[[0, 1], [2, 3]], 3, [0.5, 1.0], np.zeros((2, 1), np.int32)])
def test_wrappers_reject_malformed_nodes(no_lib, nodes):
    api = no_lib
    ctx = _bare(api.Context, handle=None, _gn_V=4)
    with pytest.raises(ValueError, match="nodes"):
        ctx.gn_marginals(nodes)
    with pytest.raises(ValueError, match="nodes"):
        ctx.marginals(np.zeros((4, 3)), np.zeros(0, api.FACTOR_DTYPE), nodes)
    inc = _bare(api.IncGraph, handle=None)
    with pytest.raises(ValueError, match="nodes"):
        inc.marginals(nodes)


@pytest.mark.parametrize("pairs", [[0, 1], [[0, 1, 2]], [[0.0, 1.0]], np.zeros((2, 2, 2), np.int32)])
def test_wrappers_reject_malformed_pairs(no_lib, pairs):
    api = no_lib
    ctx = _bare(api.Context, handle=None)
    with pytest.raises(ValueError, match="pairs"):
        ctx.gn_marginal_pairs(pairs)


def test_get_pose_covariance_needs_a_backend_method():
    """A backend without `marginals` gets an error naming the method; GpuBackend has it."""
    from dpgslam.slam import DpgSLAM, GpuBackend
    from slam_oracle import OracleSlamBackend
    assert callable(getattr(GpuBackend, "marginals"))
    s = DpgSLAM(backend=OracleSlamBackend())
    with pytest.raises(ValueError):
        s.GetPoseCovariance()              # no node yet
    s.poses = np.zeros((2, 3), np.float32)
    with pytest.raises(NotImplementedError, match="marginals"):
        s.GetPoseCovariance()
    with pytest.raises(IndexError):
        s.GetPoseCovariance(2)
