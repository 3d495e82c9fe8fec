"""Occupancy grid of the active pose graph, host side (no GPU): the numpy reference
(tests/occ_grid_ref.py) pinned by hand, the host functions of dpg_host.c (occupancy byte, box rule),
the ABI structs, the C++ adapter's grid call, and GetOccupancyGrid's errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import occ_grid_ref as R
from dpgslam import _abi
from dpgslam._abi import lib, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dpg-slam_amd", "lib")
INC = os.path.join(ROOT, "include")
ERR_ARG, ERR_SIZE = -1, -4   # DPG_ERR_ARG, DPG_ERR_SIZE (include/dpg_slam_c.h)


def test_reference_pinned_by_hand():
    """One beam of range 1.0 along +x from a lidar at (0, 0), res 0.25: nbins = 4, t = 0, .25, .5, .75
    fall in keys (0..3, 0); the end point (1, 0) is the one hit, at key (4, 0)."""
    lidar = np.array([[0.0, 0.0]], np.float32)
    end = np.array([[1.0, 0.0]], np.float32)
    ranges = np.array([1.0], np.float32)
    off = np.array([0, 1], np.int64)
    state = (np.array([3], np.uint8), np.array([0b11111], np.uint8), np.array([1], np.uint8))
    hs, ms, ns = R.grid_counts(lidar, end, ranges, off, *state, 5, 0.25)
    assert hs == {(4, 0): 1}
    assert ms == {(0, 0): 1, (1, 0): 1, (2, 0): 1, (3, 0): 1}
    assert ns == 4
    H, M, D, _ = R.reference_grid((lidar, end), ranges, off, state, 5, 0.25, (0, 0, 5, 1))
    assert np.array_equal(H, np.array([[0, 0, 0, 0, 1]], np.int32))
    assert np.array_equal(M, np.array([[1, 1, 1, 1, 0]], np.int32))
    assert np.array_equal(D, np.array([[0, 0, 0, 0, 100]], np.int8))
    # a MAX_RANGE or REMOVED label: free samples, no hit; the sample rule needs no exclusion then
    for lab in (R.L_MAX_RANGE, R.L_REMOVED):
        hs, ms, _ = R.grid_counts(lidar, end, ranges, off, np.array([lab], np.uint8), state[1], state[2], 5, 0.25)
        assert hs == {} and ms == {(0, 0): 1, (1, 0): 1, (2, 0): 1, (3, 0): 1}
    # an inactive sector or node: nothing
    assert R.grid_counts(lidar, end, ranges, off, state[0], np.array([0b11110], np.uint8), state[2], 5, 0.25)[:2] == ({}, {})
    assert R.grid_counts(lidar, end, ranges, off, state[0], state[1], np.array([0], np.uint8), 5, 0.25)[:2] == ({}, {})
    # halves round away from zero, both signs (np.round would give 0, 2, -0, -2)
    assert R.cell_key(np.array([0.125, 0.375, 0.625, -0.125, -0.375], np.float32), 0.25).tolist() == [1, 2, 3, -1, -2]
    # a range below half a cell: nbins = 0, one sample at t = 0; the hit cell swallows it
    hs, ms, ns = R.grid_counts(lidar, np.array([[0.01, 0.0]], np.float32), np.array([0.01], np.float32), off, *state, 5, 0.25)
    assert hs == {(0, 0): 1} and ms == {} and ns == 1


def _occ(hits, misses):
    h = np.ascontiguousarray(hits, np.int32)
    m = np.ascontiguousarray(misses, np.int32)
    out = np.full(len(h), 77, np.int8)
    lib().dpg_occupancy_from_counts(ptr(h, C.c_int32), ptr(m, C.c_int32), len(h), ptr(out, C.c_int8))
    return out


def test_occupancy_from_counts():
    # n = 0 unknown; no hit 0; no miss 100; half-up: (1, 7) -> 12.5 -> 13, (1, 2) -> 33.33 -> 33
    hits = [0, 0, 5, 1, 1, 1, 3]
    misses = [0, 9, 0, 7, 2, 1, 1]
    assert _occ(hits, misses).tolist() == [-1, 0, 100, 13, 33, 50, 75]
    rng = np.random.default_rng(5)
    h = rng.integers(0, 2000, 5000).astype(np.int32)
    m = rng.integers(0, 2000, 5000).astype(np.int32)
    h[:50] = 0
    m[:25] = 0
    got = _occ(h, m)
    assert np.array_equal(got, R.occupancy(h, m))
    assert got.min() == -1 and got.max() == 100
    big = _occ([2**31 - 1, 2**31 - 1, 1], [2**31 - 1, 0, 2**31 - 1])     # the formula runs in 64 bits
    assert big.tolist() == [50, 100, 0]


def _box(lidar, r, active, res, margin):
    xy = np.ascontiguousarray(lidar, np.float32).reshape(-1, 2)
    rv = np.ascontiguousarray(r, np.float32)
    act = None if active is None else np.ascontiguousarray(active, np.uint8)
    box = np.full(4, -7, np.int32)
    rc = lib().dpg_grid_box(ptr(xy, C.c_float), ptr(rv, C.c_float), ptr(act, C.c_uint8), len(rv), res, margin,
                            ptr(box, C.c_int32))
    return rc, box.tolist()


def test_grid_box_known_answers():
    # x0 = floor(-1 / .25) - 1 = -5, x1 = ceil(1 / .25) + 1 = 5
    assert _box([[0, 0]], [1.0], None, 0.25, 1) == (0, [-5, -5, 11, 11])
    assert _box([[0, 0]], [1.0], [1], 0.25, 0) == (0, [-4, -4, 9, 9])
    # negative coordinates: x in [-10.75, -9.75] -> keys -43..-39, y in [-3, -2] -> keys -12..-8, margin 2
    assert _box([[-10.25, -2.5]], [0.5], None, 0.25, 2) == (0, [-45, -14, 9, 9])
    # float32 inputs widened to fp64: -10.3f - 0.5 = -10.8000001907..., / 0.1 lies just below -108
    assert _box([[-10.3, -2.2]], [0.5], None, 0.1, 0) == (0, [-109, -28, 12, 12])
    # the inactive node does not count, whatever it holds; two active nodes span both
    assert _box([[0, 0], [np.nan, 1e30]], [1.0, np.inf], [1, 0], 0.25, 1) == (0, [-5, -5, 11, 11])
    assert _box([[0, 0], [3, -2]], [1.0, 2.0], [1, 1], 0.5, 1) == (0, [-3, -9, 15, 13])
    assert _box([[0, 0], [3, -2]], [1.0, 2.0], [0, 1], 0.5, 1) == (0, [1, -9, 11, 11])
    # no active node: w = h = 0 and success
    assert _box([[0, 0], [3, -2]], [1.0, 2.0], [0, 0], 0.5, 1) == (0, [0, 0, 0, 0])
    assert _box(np.zeros((0, 2)), np.zeros(0), None, 0.5, 1) == (0, [0, 0, 0, 0])
    # errors: resolution, margin, a non-finite active node, a key beyond +-2^29
    assert _box([[0, 0]], [1.0], None, 0.0, 1)[0] == ERR_ARG
    assert _box([[0, 0]], [1.0], None, float("nan"), 1)[0] == ERR_ARG
    assert _box([[0, 0]], [1.0], None, 0.25, -1)[0] == ERR_ARG
    assert _box([[np.nan, 0]], [1.0], None, 0.25, 1)[0] == ERR_ARG
    assert _box([[1e9, 0]], [1.0], None, 0.25, 1)[0] == ERR_SIZE


def test_grid_params_default():
    p = _abi.default_grid_params()
    assert (p.resolution, p.max_cells, p.margin_cells, p.pad) == (0.0, 0, 1, 0)


def test_grid_struct_sizes_match_the_header(tmp_path):
    txt = open(os.path.join(INC, "dpg_slam_c.h")).read()
    sizes = {k: int(v) for k, v in re.findall(r"#define (DPG_GRID_(?:PARAMS|INFO)_SIZE) (\d+)", txt)}
    assert len(re.findall(r"_Static_assert\(sizeof\(dpg_grid_params\) == DPG_GRID_PARAMS_SIZE && "
                          r"sizeof\(dpg_grid_info\) == DPG_GRID_INFO_SIZE", txt)) == 1
    assert C.sizeof(_abi.GridParams) == sizes["DPG_GRID_PARAMS_SIZE"]
    assert C.sizeof(_abi.GridInfo) == sizes["DPG_GRID_INFO_SIZE"]
    # the header compiles as C (its static assertion holds) and the field offsets agree
    for struct, cls in (("dpg_grid_params", _abi.GridParams), ("dpg_grid_info", _abi.GridInfo)):
        names = [f[0] for f in cls._fields_]
        body = "".join(f'printf(" %zu", offsetof({struct}, {f}));' for f in names)
        src = tmp_path / f"{struct}.c"
        src.write_text(f'#include <stddef.h>\n#include <stdio.h>\n#include "dpg_slam_c.h"\n'
                       f'int main(void) {{ printf("%zu", sizeof({struct})); {body} return 0; }}\n')
        exe = str(tmp_path / struct)
        subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", INC, "-o", exe, str(src)], check=True)
        lay = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
        assert lay[0] == C.sizeof(cls)
        assert lay[1:] == [getattr(cls, n).offset for n in names]


def test_adapter_grid_check_compiles_and_links(tmp_path):
    out = str(tmp_path / "adapter_grid_check")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + INC, "-o", out,
                        os.path.join(ROOT, "tools", "adapter_grid_check.cpp"), "-L" + LIBDIR, "-ldpg"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


class _NoGridStore:
    pass


class _Backend:
    def store(self, ranges, geom, offsets, params):
        return _NoGridStore()


def test_get_occupancy_grid_errors():
    from dpgslam.slam import DpgSLAM
    s = DpgSLAM(backend=_Backend())
    with pytest.raises(ValueError, match="no node"):
        s.GetOccupancyGrid()
    s.poses = np.zeros((1, 3), np.float32)
    s.ranges = [np.ones(4, np.float32)]
    s.geom = [(-1.0, 1.0, 8.0)]
    with pytest.raises(NotImplementedError, match="occupancy_grid"):
        s.GetOccupancyGrid()
    with pytest.raises(ValueError, match="resolution"):
        s.GetOccupancyGrid(-0.1)
