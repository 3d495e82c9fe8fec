"""Occupancy grid of the active pose graph on the GPU (dpg_occupancy_grid, csrc/dpg_grid.hip)
against the numpy restatement tests/occ_grid_ref.py: hits, misses and the occupancy byte of EVERY
cell of the returned box are equal, no tolerance; every cell the reference marks lies inside the box
and the kernel reports no sample outside it.  The reference takes the device's own lidar positions
and beam end points (dpg_dpg_beam_geometry), which test k pins against the oracle-pinned map lists."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import occ_grid_ref as R
from dpgslam import _abi, api, synth
from dpgslam._abi import lib, ptr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dpg-slam_amd", "lib")
L_STATIC, L_ADDED, L_REMOVED, L_NYL, L_MAX = 0, 1, 2, 3, 4
NB = 360
AMIN, AMAX = -math.pi, math.pi
ERR_SIZE = -4   # DPG_ERR_SIZE
N_VARIANTS = 10  # raster kernel variants selectable through dpg_grid_params.pad (0 = the product)


def _geom(n, rmax=8.0, amin=AMIN, amax=AMAX):
    return np.tile(np.array([amin, amax, rmax], np.float32), (n, 1))


def _params(res=0.0, **kw):
    p = _abi.default_grid_params()
    p.resolution = res
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _check(store, n_nodes, est, ranges, res=0.0, num_sectors=5, **kw):
    """The grid of `store` equals the reference on the store's fetched state; returns the grid."""
    g = store.occupancy_grid(n_nodes, est, _params(res, **kw), counts=True)
    info = g["info"]
    box = (info.x0, info.y0, info.w, info.h)
    assert (g["height"], g["width"]) == (info.h, info.w) == g["data"].shape
    assert g["origin"] == ((info.x0 - 0.5) * g["resolution"], (info.y0 - 0.5) * g["resolution"])
    geo = store.beam_geometry(n_nodes, est)
    H, M, D, ns = R.reference_grid(geo, np.asarray(ranges, np.float32).reshape(-1), store.offsets, store.fetch(),
                                   num_sectors, g["resolution"], box)       # asserts: every marked cell in the box
    print(f"grid {info.w} x {info.h} res {g['resolution']}: hits {info.n_hits} samples {info.n_samples} "
          f"direct {info.n_direct} flushed {info.n_flushed} oob {info.n_oob} kernels {info.ms_kernels:.3f} ms")
    np.testing.assert_array_equal(g["hits"], H)
    np.testing.assert_array_equal(g["misses"], M)
    np.testing.assert_array_equal(g["data"], D)
    assert info.n_oob == 0
    assert info.n_samples == ns and info.n_hits == int(H.sum())
    return g


def _ring(extra_sector_range=None):
    r = np.full((2, NB), 5.0, np.float32)
    if extra_sector_range is not None:
        r[1, :72] = extra_sector_range
    return r, _geom(2)


def test_a_ring_rotated_negative(ctx):
    r, geom = _ring()
    est = np.array([[-3.25, -7.5, 0.3], [-2.5, -8.1, -2.1]], np.float32)
    s = api.DpgStore(ctx, r, geom)
    g = _check(s, 2, est, r)
    assert g["resolution"] == 0.05 and g["info"].n_nodes_used == 2 and g["info"].n_beams_used == 2 * NB
    assert g["info"].n_hits == 2 * NB and (g["data"] == 100).any() and (g["data"] == 0).any() and (g["data"] == -1).any()
    assert g["origin"][0] < -8 and g["origin"][1] < -13
    _check(s, 2, est, r, res=0.1)
    _check(s, 1, est, r, res=0.1)          # a prefix of the nodes
    s.close()


def test_b_node_state(ctx):
    r, geom = _ring(extra_sector_range=7.0)
    est = np.zeros((2, 3), np.float32)
    s = api.DpgStore(ctx, r, geom)
    st = s.execute_dpg(2, 1, est)
    lab, sec, act = s.fetch()
    assert st.n_removed > 0 and not (sec[0] & 1) and (lab == L_REMOVED).any()
    g = _check(s, 2, est, r)
    # the REMOVED points' sector (sector 0 of node 0) contributes nothing
    inc = R.included_beams(s.offsets, lab, sec, act, 5)
    assert not inc[:72].any() and inc[72:].all() and g["info"].n_beams_used == int(inc.sum())
    assert g["info"].n_hits == int(inc.sum())       # the REMOVED labels all sit in the inactive sector
    box2 = (g["info"].x0, g["info"].y0, g["info"].w, g["info"].h)
    # node 0 dropped entirely: the box is node 1's alone (largest range 7 around its lidar)
    s.load(node_active=np.array([0, 1], np.uint8))
    g1 = _check(s, 2, est, r)
    lidar, _ = s.beam_geometry(2, est)
    want = np.zeros(4, np.int32)
    rv = np.array([7.0], np.float32)
    assert lib().dpg_grid_box(ptr(np.ascontiguousarray(lidar[1:2]), C.c_float), ptr(rv, C.c_float), None, 1, 0.05, 1,
                              ptr(want, C.c_int32)) == 0
    assert (g1["info"].x0, g1["info"].y0, g1["info"].w, g1["info"].h) == tuple(want.tolist()) == box2
    assert g1["info"].n_nodes_used == 1 and g1["info"].n_beams_used == NB
    s.load(node_active=np.array([1, 0], np.uint8))   # node 0 alone (range 5): the box shrinks
    g0 = _check(s, 2, est, r)
    assert g0["info"].w < g1["info"].w and g0["info"].n_beams_used == NB - 72
    # a REMOVED label in a still active sector: its free samples count, its end point does not
    s.load(node_active=np.array([1, 1], np.uint8))
    lab2 = lab.copy()
    lab2[NB + 200] = L_REMOVED
    s.load(labels=lab2)
    g2 = _check(s, 2, est, r)
    assert g2["info"].n_hits == g["info"].n_hits - 1 and g2["info"].n_samples == g["info"].n_samples
    assert int(g2["misses"].sum()) >= int(g["misses"].sum())
    s.close()


def test_c_table_overflow_and_variants(ctx):
    """64 beams of 30 m at res 0.05: 600 samples per beam, all 64 beams in one workgroup (128 beams of
    8 lanes) -- several times the distinct cells the 8192-slot LDS table holds, so adds go straight to
    the global counters; every kernel variant (other tables, lane groups, workgroups, no table at
    all) gives the same grid."""
    r = np.full((1, 64), 30.0, np.float32)
    geom = _geom(1, rmax=40.0)
    est = np.array([[1.3, -0.7, 0.4]], np.float32)
    s = api.DpgStore(ctx, r, geom)
    g = _check(s, 1, est, r)
    assert g["info"].n_direct > 0 and g["info"].n_flushed > 0
    for v in range(1, N_VARIANTS):
        gv = s.occupancy_grid(1, est, _params(pad=v), counts=True)
        np.testing.assert_array_equal(gv["hits"], g["hits"], err_msg=f"variant {v}")
        np.testing.assert_array_equal(gv["misses"], g["misses"], err_msg=f"variant {v}")
        np.testing.assert_array_equal(gv["data"], g["data"], err_msg=f"variant {v}")
        assert gv["info"].n_samples == g["info"].n_samples and gv["info"].n_oob == 0
        if v == 7:    # no table: every hit and every counted sample is one global add
            assert gv["info"].n_flushed == 0 and gv["info"].n_direct == gv["info"].n_samples + 64 - _own_cell(g)
    with pytest.raises(_abi.DpgError):
        s.occupancy_grid(1, est, _params(pad=N_VARIANTS))
    s.close()


def _own_cell(g):
    """Samples dropped because they fell in their own beam's hit cell: marched minus counted."""
    return int(g["info"].n_samples) - int(g["misses"].sum())


def test_d_heavy_sharing(ctx):
    r = np.full((1, NB), 5.0, np.float32)
    est = np.array([[0.3, -0.2, 1.0]], np.float32)
    s = api.DpgStore(ctx, r, _geom(1))
    g1 = _check(s, 1, est, r, res=1.0)
    assert g1["misses"].max() > 100          # hundreds of rays through the cells at the lidar
    s.close()
    r40 = np.full((40, NB), 5.0, np.float32)
    est40 = np.tile(est, (40, 1))
    s = api.DpgStore(ctx, r40, _geom(40))
    g40 = _check(s, 40, est40, r40, res=1.0)
    np.testing.assert_array_equal(g40["hits"], 40 * g1["hits"])
    np.testing.assert_array_equal(g40["misses"], 40 * g1["misses"])
    np.testing.assert_array_equal(g40["data"], g1["data"])
    s.close()


def test_e_exact_ties(ctx):
    """Laser at the base_link origin, pose (0.125, 0.375, 0), res 0.25, beams at 0 and pi/2: the keys
    are exact halves (0.5, 1.5, ...), rounded away from zero."""
    p = _abi.default_change_params()
    p.laser[0] = p.laser[1] = p.laser[2] = 0.0
    r = np.array([[1.0, 1.0]], np.float32)
    geom = _geom(1, amin=0.0, amax=math.pi / 2)
    est = np.array([[0.125, 0.375, 0.0]], np.float32)
    s = api.DpgStore(ctx, r, geom, params=p)
    g = _check(s, 1, est, r, res=0.25)
    lidar, end = s.beam_geometry(1, est)
    assert lidar.tolist() == [[0.125, 0.375]] and end[0].tolist() == [1.125, 0.375]
    x0, y0 = g["info"].x0, g["info"].y0
    # beam 0: samples at x = .125, .375, .625, .875 (keys 1, 2, 3, 4: halves go up), y = .375 (key 2); hit at (5, 2)
    assert [int(g["misses"][2 - y0, k - x0]) for k in (1, 2, 3, 4)] == [2, 1, 1, 1]   # (1, 2) also holds beam 1's t = 0
    assert g["hits"][2 - y0, 5 - x0] == 1 and g["misses"][2 - y0, 0 - x0] == 0
    for q in (-1.0, 1.0):   # mirrored: negative halves round down
        e2 = np.array([[q * 0.125, -0.375, 0.0]], np.float32)
        _check(s, 1, e2, r, res=0.25)
    s.close()


def test_f_degenerate_beams(ctx):
    """Ranges 0 and 0.01 (nbins = 0: one sample at t = 0), 0.03, and one at range_max (label MAX_RANGE:
    free samples, no hit) in one scan."""
    r = np.array([[0.0, 0.01, 0.03, 9.0, 2.0, 8.0]], np.float32)
    est = np.array([[-0.4, 0.9, 2.5]], np.float32)
    s = api.DpgStore(ctx, r, _geom(1, rmax=8.0))
    lab = s.fetch()[0]
    assert lab.tolist() == [L_NYL, L_NYL, L_NYL, L_MAX, L_NYL, L_MAX]
    g = _check(s, 1, est, r)
    assert g["info"].n_hits == 4 and g["info"].n_beams_used == 6
    # one sample each for the ranges 0, 0.01 and 0.03 (nbins 0, 0, 1), then 180, 40 and 160 bins (one
    # more sample where the float t chain ends just below 1)
    assert 3 + 180 + 40 + 160 <= g["info"].n_samples <= 3 + 181 + 41 + 161
    _check(s, 1, est, r, res=0.013)
    s.close()


def test_g_ragged_store_and_regrow(ctx):
    rng = np.random.default_rng(11)
    sizes = [2, 33, 360]        # the store takes no scan of fewer than 2 beams (dpg_dpg_create)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    r = rng.uniform(0.5, 6.0, int(off[-1])).astype(np.float32)
    est = np.array([[0.0, 0.0, 0.0], [-1.5, 2.0, 1.0], [3.0, -2.5, -0.5], [9.0, 7.0, 2.0]], np.float32)
    with pytest.raises(_abi.DpgError):
        api.DpgStore(ctx, np.ones(1, np.float32), _geom(1), offsets=np.array([0, 1], np.int64))
    s = api.DpgStore(ctx, r, _geom(3), offsets=off)
    g3 = _check(s, 3, est[:3], r)
    r4 = rng.uniform(0.5, 7.5, 1000).astype(np.float32)
    s.append(r4, _geom(1), offsets=np.array([0, 1000], np.int64))
    rr = np.concatenate([r, r4])
    g4 = _check(s, 4, est, rr)           # a larger box and more beams: the buffers regrow
    assert g4["info"].w > g3["info"].w and g4["info"].n_beams_used == 1395
    g3b = _check(s, 3, est[:3], rr)      # and the smaller request again, in the larger buffers
    np.testing.assert_array_equal(g3b["misses"], g3["misses"])
    _check(s, 4, est, rr, res=0.1)
    s.close()


def _dynamic():
    return synth.make_dynamic(n_passes=3, nodes_per_pass=20, n_beams=NB, world_size=20.0, range_max=8.0, n_boxes=10)


def test_h_through_dpgslam():
    from dpgslam.slam import DpgSLAM
    w = _dynamic()
    own = api.Context(0)          # the run fills its context's scan store: keep the shared one as it is
    slam = DpgSLAM(ctx=own)
    rng = np.random.default_rng(3)
    for p in range(len(w.pass_start) - 1):
        if p:
            slam.incrementPassNumber()
        for v in range(int(w.pass_start[p]), int(w.pass_start[p + 1])):
            odom = w.est[v].astype(np.float64) + rng.normal(0, [0.01, 0.01, 0.002])
            slam.ObserveOdometry(odom[:2].astype(np.float32), np.float32(odom[2]))
            slam.ObserveLaser(w.ranges[v], 0.0, float(w.geom[v, 2]), float(w.geom[v, 0]), float(w.geom[v, 1]))
    V = len(slam.poses)
    assert V > 30
    store = slam._dpg_store()
    ranges = np.concatenate(slam.ranges)
    lab, sec, act = store.fetch()
    assert (lab == L_REMOVED).any() or (lab == L_ADDED).any()
    for res in (None, 0.1):
        grid = slam.GetOccupancyGrid() if res is None else slam.GetOccupancyGrid(res)
        assert set(grid) == {"resolution", "origin", "width", "height", "data"}
        assert grid["resolution"] == (0.05 if res is None else 0.1)
        g = _check(store, V, slam.poses, ranges, res=0.0 if res is None else res)
        np.testing.assert_array_equal(grid["data"], g["data"])
        assert grid["origin"] == g["origin"] and (grid["height"], grid["width"]) == g["data"].shape
        assert g["info"].n_nodes_used == int(act.sum())
    own.close()


def test_i_no_side_effects(ctx):
    """The change detection run twice over the same workload, once with a grid call before every
    executeDPG: identical counters and node state after every call; two grid calls are bitwise equal."""
    w = _dynamic()
    a = api.DpgStore(ctx, w.ranges, w.geom)
    b = api.DpgStore(ctx, w.ranges, w.geom)
    n0 = int(w.pass_start[1])
    for v in range(n0, w.V):
        cur = int(v - w.pass_start[w.pass_of[v]] + 1)
        est = w.est[:v + 1]
        g1 = b.occupancy_grid(v + 1, est, counts=True)
        if v % 8 == 0:
            g2 = b.occupancy_grid(v + 1, est, counts=True)
            for k in ("hits", "misses", "data"):
                assert g1[k].tobytes() == g2[k].tobytes(), (v, k)
        sa, sb = a.execute_dpg(v + 1, cur, est), b.execute_dpg(v + 1, cur, est)
        assert sa.counters() == sb.counters(), (v, sa.counters(), sb.counters())
        assert sa.grid_cells == sb.grid_cells and sa.n_samples == sb.n_samples, v   # the kept window and planes too
        for x, y in zip(a.fetch(), b.fetch()):
            assert np.array_equal(x, y), v
    _check(b, w.V, w.est, w.ranges)
    la, lb = a.active_dynamic_points(w.V, w.est), b.active_dynamic_points(w.V, w.est)
    for k in la:
        assert np.array_equal(la[k], lb[k]), k
    a.close()
    b.close()


def _raw(store, n, est, p, hits, misses, occ, cap):
    info = _abi.GridInfo()
    e = np.ascontiguousarray(est, np.float32)
    rc = lib().dpg_occupancy_grid(store.handle, n, ptr(e, C.c_float), C.byref(p), ptr(hits, C.c_int32),
                                  ptr(misses, C.c_int32), ptr(occ, C.c_int8), cap, C.byref(info))
    return rc, info


def test_j_errors_and_plan(ctx):
    r, geom = _ring()
    est = np.array([[-3.25, -7.5, 0.3], [-2.5, -8.1, -2.1]], np.float32)
    s = api.DpgStore(ctx, r, geom)
    p = _params()
    rc, plan = _raw(s, 2, est, p, None, None, None, 0)           # plan only
    assert rc == 0 and plan.w > 0 and plan.h > 0
    assert plan.ms_kernels == 0.0 and plan.n_samples == 0 and plan.n_beams_used == 0 and plan.n_nodes_used == 2
    cells = plan.w * plan.h
    hits, misses = np.full(cells, 12345, np.int32), np.full(cells, 12345, np.int32)
    occ = np.full(cells, 77, np.int8)
    for outs in ((hits, misses, occ), (hits, None, None), (None, None, occ)):
        rc, _ = _raw(s, 2, est, p, *outs, cells - 1)              # cap one short: nothing written
        assert rc == ERR_SIZE
        assert (hits == 12345).all() and (misses == 12345).all() and (occ == 77).all()
    rc, _ = _raw(s, 2, est, _params(max_cells=16), hits, misses, occ, cells)
    assert rc == ERR_SIZE and (hits == 12345).all() and (occ == 77).all()
    assert _raw(s, 2, est, _params(max_cells=16), None, None, None, 0)[0] == ERR_SIZE
    rc, fill = _raw(s, 2, est, p, hits, misses, occ, cells)
    assert rc == 0 and (fill.x0, fill.y0, fill.w, fill.h) == (plan.x0, plan.y0, plan.w, plan.h)
    assert fill.n_samples > 0 and not (hits == 12345).any() and not (occ == 77).any()
    rc, _ = _raw(s, 2, est, p, None, None, occ, cells)             # any subset of the outputs
    assert rc == 0
    host = np.zeros(cells, np.int8)
    lib().dpg_occupancy_from_counts(ptr(hits, C.c_int32), ptr(misses, C.c_int32), cells, ptr(host, C.c_int8))
    assert np.array_equal(host, occ)
    # no active node: an empty grid, and success
    s.load(node_active=np.array([0, 0], np.uint8))
    g = s.occupancy_grid(2, est, counts=True)
    assert (g["width"], g["height"]) == (0, 0) and g["data"].shape == (0, 0) and g["info"].n_nodes_used == 0
    # bad arguments
    assert _raw(s, 3, est, p, None, None, None, 0)[0] == -1 and _raw(s, 2, est, _params(-1.0), None, None, None, 0)[0] == -1
    assert _raw(s, 2, est, _params(margin_cells=-1), None, None, None, 0)[0] == -1
    # beam geometry: a short end_xy is refused with nothing written
    end = np.full((2 * NB, 2), 7.0, np.float32)
    e = np.ascontiguousarray(est)
    assert lib().dpg_dpg_beam_geometry(s.handle, 2, ptr(e, C.c_float), None, ptr(end, C.c_float), 2 * NB - 1) == ERR_SIZE
    assert (end == 7.0).all()
    s.close()


def test_k_beam_geometry_matches_map_lists(ctx):
    rng = np.random.default_rng(4)
    r = rng.uniform(1.0, 7.9, (3, NB)).astype(np.float32)
    est = np.array([[-3.25, -7.5, 0.3], [-2.5, -8.1, -2.1], [4.0, 1.0, 3.0]], np.float32)
    s = api.DpgStore(ctx, r, _geom(3))
    lab = rng.integers(0, 4, 3 * NB).astype(np.uint8)       # STATIC, ADDED, REMOVED, NOT_YET_LABELED
    s.load(labels=lab)
    lidar, end = s.beam_geometry(3, est)
    lists = s.active_dynamic_points(3, est)
    assert lists["active_static"].tobytes() == end[lab == L_STATIC].tobytes()
    assert lists["active_added"].tobytes() == end[lab == L_ADDED].tobytes()
    assert lists["dynamic_removed"].tobytes() == end[lab == L_REMOVED].tobytes()
    assert lists["dynamic_added"].tobytes() == end[lab == L_ADDED].tobytes()
    assert len(lists["active_static"]) > 100
    # the lidar sits laser[0] = 0.2 m ahead of the node; a prefix of the nodes gives a prefix of the beams
    np.testing.assert_allclose(np.hypot(*(lidar - est[:, :2]).T), 0.2, atol=1e-5)
    l2, e2 = s.beam_geometry(2, est[:2])
    assert l2.tobytes() == lidar[:2].tobytes() and e2.tobytes() == end[:2 * NB].tobytes()
    s.close()


def test_adapter_grid_check_runs(tmp_path):
    exe = str(tmp_path / "adapter_grid_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(ROOT, "tools", "adapter_grid_check.cpp"), "-L" + LIBDIR, "-ldpg"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, LD_LIBRARY_PATH=LIBDIR))
    print(r.stdout)
    assert r.returncode == 0 and "adapter grid check ok" in r.stdout, r.stdout + r.stderr
