"""Localisation of one scan in the active map on the GPU (dpg_map_localize and its diagnostics)
against the numpy restatement tests/loc_ref.py, byte for byte: after the one float transform per
point and angle everything is integer, so no tolerance is needed or allowed.

World: csm_ref's 12 x 9 m room with three boxes, scanned from six poses (360 beams each) into a
DpgStore, at a resolution of 0.1 m; the lidar sits at the body origin, so a node's pose is its
lidar's."""
import ctypes as C
import math

import numpy as np
import pytest

import csm_ref
import loc_ref as L
from dpgslam import _abi, api, synth
from dpgslam._abi import lib, ptr

pytestmark = pytest.mark.gpu

f32 = np.float32
NB = 360
RES = 0.1
KT = 256          # threads of a workgroup of the bound kernel: a tile of 64 x 4 blocks
KCHUNK = 2048     # keys per LDS chunk of the bound kernel
AMIN, AMAX = -math.pi, -math.pi + (NB - 1) * 2.0 * math.pi / NB
RMAX = 30.0
NODE_POSES = [(2.0, 2.0, 0.3), (5.5, 1.2, 1.9), (10.5, 2.0, -2.5), (10.0, 7.0, 0.8), (5.0, 7.5, -1.0), (1.5, 6.5, 2.6)]
QUERY_POSE = (6.43, 4.57, 1.106)          # off the cell centres and the angle steps


def _params(**kw):
    p = _abi.default_loc_params()
    p.resolution = RES
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class World:
    def __init__(self):
        rng = np.random.default_rng(4711)
        segs = csm_ref._segments()
        self.est = np.array(NODE_POSES, f32)
        self.clouds = [csm_ref._scan(p, segs, NB, 0.01, rng) for p in NODE_POSES]
        self.ranges = np.stack([np.hypot(c[:, 0].astype(np.float64), c[:, 1].astype(np.float64)) for c in self.clouds]).astype(f32)
        self.geom = np.tile(np.array([AMIN, AMAX, RMAX], f32), (len(NODE_POSES), 1))
        q = csm_ref._scan(QUERY_POSE, segs, NB, 0.01, rng)
        self.query_ranges = np.hypot(q[:, 0].astype(np.float64), q[:, 1].astype(np.float64)).astype(f32)
        self.query = api.scan_to_cloud(self.query_ranges, f32(AMIN), f32(AMAX), f32(RMAX), (0.0, 0.0, 0.0))
        self.V = len(NODE_POSES)

    def store(self, ctx):
        cp = _abi.default_change_params()
        cp.laser[0] = cp.laser[1] = cp.laser[2] = 0.0
        return api.DpgStore(ctx, self.ranges, self.geom, params=cp)


_WORLD = None


def world() -> World:
    global _WORLD
    if _WORLD is None:
        _WORLD = World()
    return _WORLD


@pytest.fixture(scope="module")
def room_store(ctx):
    s = world().store(ctx)
    yield s
    s.close()


_OCC = {}


def _occ(store, key="all"):
    """The store's occupancy bytes and box for the test resolution (computed once per node state)."""
    if key not in _OCC:
        w = world()
        gp = _abi.default_grid_params()
        gp.resolution = RES
        g = store.occupancy_grid(w.V, w.est, gp, counts=True)
        _OCC[key] = (g["data"].copy(), (g["info"].x0, g["info"].y0, g["info"].w, g["info"].h))
    return _OCC[key]


def _problem(store, cloud, guess, p, key="all"):
    occ, box = _occ(store, key)
    return L.Problem(occ, box, RES, cloud, guess, p)


def _winner(r):
    return int(r["score"]), int(r["best_a"]), int(r["best_dx"]), int(r["best_dy"])


# ------------------------------------------------------------------ field
def _check_fields(store, key, **kw):
    w = world()
    occ, box = _occ(store, key)
    p = _params(**kw)
    F, gbox = store.map_field(w.V, w.est, p)
    assert gbox == box and F.shape == occ.shape
    want = L.field(occ, p, RES)
    assert F.tobytes() == want.tobytes()
    for shift in (0, 1, 3):
        P, _ = store.map_field(w.V, w.est, p, shift=shift)
        assert P.shape == (box[3] + (1 << shift) - 1, box[2] + (1 << shift) - 1)
        assert P.tobytes() == L.pooled(want, shift).tobytes(), shift
    return want


def test_field_equals_the_reference(room_store):
    F = _check_fields(room_store, "all")
    assert (F == 255).sum() > 200 and (F == 0).sum() > F.size // 2 and F.shape[0] * F.shape[1] > 256 * 64
    lo = _check_fields(room_store, "all", occupied_min=1)
    hi = _check_fields(room_store, "all", occupied_min=100)
    assert (lo >= F).all() and (F >= hi).all() and (lo > hi).any()
    _check_fields(room_store, "all", kernel_radius=0)
    _check_fields(room_store, "all", kernel_radius=7, sigma=0.35)


def test_field_follows_the_node_state(ctx):
    w = world()
    s = w.store(ctx)
    act = np.ones(w.V, np.uint8)
    act[2] = 0
    sec = np.full(w.V, 0b11111, np.uint8)
    sec[0], sec[4] = 0b01010, 0b00001
    s.load(sector_active=sec, node_active=act)
    F = _check_fields(s, "partial")
    assert _occ(s, "partial")[1] != _occ(s, "all")[1] or F.tobytes() != L.field(_occ(s, "all")[0], _params(), RES).tobytes()
    s.load(node_active=np.zeros(w.V, np.uint8))                       # no active node: an empty field, and a valid answer
    F0, box0 = s.map_field(w.V, w.est, _params())
    assert F0.size == 0 and box0[2:] == (0, 0)
    r = s.localize(w.V, w.est, w.query, (1.0, 2.0, 0.5), _params(half_x=3, half_y=2, half_a=1))
    want = L.Problem(np.zeros((0, 0), np.int8), box0, RES, w.query, (1.0, 2.0, 0.5), _params(half_x=3, half_y=2, half_a=1)).search()
    assert L.same_record(r, want) and int(r["status"]) == _abi.DPG_LOC_NO_OVERLAP
    assert not s.localize_bounds(w.V, w.est, w.query, (1.0, 2.0, 0.5), _params(half_x=3, half_y=2, half_a=1)).any()
    s.close()


# ------------------------------------------------------------------ bounds and scores
def _check_volumes(store, cloud, guess, p):
    w = world()
    P = _problem(store, cloud, guess, p)
    b = store.localize_bounds(w.V, w.est, cloud, guess, p)
    v = store.localize_scores(w.V, w.est, cloud, guess, p)
    wb, wv = P.bounds(), P.scores()
    assert b.shape == wb.shape and b.tobytes() == wb.tobytes()
    assert v.shape == wv.shape and v.tobytes() == wv.tobytes()
    s = P.s
    pad = np.full((P.A, P.nby * s, P.nbx * s), -1, np.int64)
    pad[:, :v.shape[1], :v.shape[2]] = v
    blockmax = pad.reshape(P.A, P.nby, s, P.nbx, s).max((2, 4))
    assert (b >= blockmax).all()
    return P, b, v


def _guess_near_truth():
    return (QUERY_POSE[0] + 0.33, QUERY_POSE[1] - 0.21, QUERY_POSE[2] + 0.04)


@pytest.mark.parametrize("n", [0, 1, 65, KCHUNK + 1])
def test_volumes_by_cloud_size(room_store, n):
    w = world()
    rng = np.random.default_rng(n)
    cloud = np.concatenate([w.query] * (n // len(w.query) + 1))[:n] + rng.normal(0, 0.02, (n, 2)).astype(f32)
    p = _params(half_x=6, half_y=5, half_a=1, angle_step=math.radians(3), coarse_shift=2)
    P, b, v = _check_volumes(room_store, np.ascontiguousarray(cloud, f32), _guess_near_truth(), p)
    assert (v.max() > 0) == (n > 0)


def test_volumes_non_finite_and_huge_points(room_store):
    w = world()
    cloud = w.query[:90].copy()
    cloud[3] = [np.nan, 1.0]
    cloud[7] = [np.inf, -np.inf]
    cloud[11] = [3e38, 0.5]
    cloud[12] = [0.1 * 2 ** 29, 0.0]       # at the key limit
    cloud[13] = [-5.3e7, 5.3e7]            # a valid key far outside every box
    cloud[14] = [1e6, -1e6]
    p = _params(half_x=5, half_y=4, half_a=2, angle_step=math.radians(2), coarse_shift=1)
    _check_volumes(room_store, cloud, _guess_near_truth(), p)


@pytest.mark.parametrize("name,kw,guess", [
    ("ragged_row", dict(half_x=10, half_y=0, half_a=1, coarse_shift=3), None),        # 21 shifts in blocks of 8, one row
    ("single_angle", dict(half_x=7, half_y=9, half_a=0, coarse_shift=2), None),
    ("over_the_edge", dict(half_x=12, half_y=12, half_a=1, coarse_shift=3), "edge"),
    ("many_blocks", dict(half_x=80, half_y=9, half_a=0, coarse_shift=0), None),        # 161 x 19 blocks: several tiles each way
    ("shift5", dict(half_x=40, half_y=33, half_a=0, coarse_shift=5), None),
])
def test_volumes_by_window(room_store, name, kw, guess):
    w = world()
    g = _guess_near_truth()
    if guess == "edge":
        _, box = _occ(room_store)
        g = ((box[0] + 2) * RES, (box[1] + box[3] - 3) * RES, 0.4)                    # the window hangs over two edges of the box
    P, b, v = _check_volumes(room_store, w.query, g, _params(angle_step=math.radians(2), **kw))
    if name == "many_blocks":
        assert P.nbx * P.nby > KT and P.nbx > 64 and P.nby > 4


def test_window_wholly_outside_the_box(room_store):
    w = world()
    p = _params(half_x=9, half_y=9, half_a=1, coarse_shift=2)
    g = (900.0, -700.0, 0.3)
    P, b, v = _check_volumes(room_store, w.query, g, p)
    assert not b.any() and not v.any()
    r = room_store.localize(w.V, w.est, w.query, g, p)
    assert L.same_record(r, P.search()) and int(r["status"]) == _abi.DPG_LOC_NO_OVERLAP
    assert _winner(r) == (0, 1, 0, 0) and int(r["n_frontier"]) == int(r["n_blocks"])


# ------------------------------------------------------------------ winner
_BRUTE = {}


def _brute_problem(store):
    """The +-40 cell, 31 angle window around a guess near the truth, and its brute-force volume (about
    7e7 lookups in numpy, computed once)."""
    if "v" not in _BRUTE:
        p = _params(half_x=40, half_y=40, half_a=15, angle_step=math.radians(1), coarse_shift=0)
        P = _problem(store, world().query, (QUERY_POSE[0] + 1.7, QUERY_POSE[1] - 2.2, QUERY_POSE[2] + 0.13), p)
        _BRUTE["v"] = (P.guess, P.scores())
    return _BRUTE["v"]


@pytest.mark.parametrize("shift", [0, 1, 3, 4])   # at 4 the frontier holds several blocks
def test_winner_equals_brute_force(room_store, shift):
    w = world()
    guess, vol = _brute_problem(room_store)
    p = _params(half_x=40, half_y=40, half_a=15, angle_step=math.radians(1), coarse_shift=shift)
    P = _problem(room_store, w.query, guess, p)
    r = room_store.localize(w.V, w.est, w.query, guess, p)
    assert _winner(r) == P.brute(vol) and int(r["status"]) == _abi.DPG_LOC_OK
    assert int(r["score_at_guess"]) == int(vol[15, 40, 40])
    want = P.search()
    assert L.same_record(r, want), (r, want)
    # the winner is the query's pose to within a cell and a step
    assert abs(float(r["pose"][0]) - QUERY_POSE[0]) <= RES and abs(float(r["pose"][1]) - QUERY_POSE[1]) <= RES
    assert abs(float(r["pose"][2]) - QUERY_POSE[2]) <= math.radians(1)
    r2 = room_store.localize(w.V, w.est, w.query, guess, p)
    assert all(r[n].tobytes() == r2[n].tobytes() for n in _abi.LOC_RESULT_EXACT)
    print(f"shift {shift}: score {int(r['score'])} of {255 * NB}, frontier {int(r['n_frontier'])} of {int(r['n_blocks'])} blocks, "
          f"{int(r['n_refined_candidates'])} candidates refined; field {float(r['ms_field']):.3f} bound {float(r['ms_bound']):.3f} "
          f"fine {float(r['ms_fine']):.3f} ms")


def test_tie_order_in_a_symmetric_room(ctx):
    """A square room scanned from its centre, searched over the full circle at 90-degree steps: a = 0
    and a = 4 are the same rotation up to the sign of a sine of 8.7e-8, so their scores tie."""
    n = 360
    ang = AMIN + np.arange(n) * (AMAX - AMIN) / (n - 1)
    r = (4.0 / np.maximum(np.abs(np.cos(ang)), np.abs(np.sin(ang)))).astype(f32)
    cp = _abi.default_change_params()
    cp.laser[0] = cp.laser[1] = cp.laser[2] = 0.0
    geom = np.array([[AMIN, AMAX, RMAX]], f32)
    est = np.zeros((1, 3), f32)
    s = api.DpgStore(ctx, r[None, :], geom, params=cp)
    gp = _abi.default_grid_params()
    gp.resolution = RES
    g = s.occupancy_grid(1, est, gp, counts=True)
    box = (g["info"].x0, g["info"].y0, g["info"].w, g["info"].h)
    cloud = api.scan_to_cloud(r, f32(AMIN), f32(AMAX), f32(RMAX), (0.0, 0.0, 0.0))
    for shift in (0, 3):
        p = _params(half_x=5, half_y=5, half_a=2, angle_step=math.pi / 2, coarse_shift=shift)
        guess = (0.2, -0.1, math.pi)
        P = L.Problem(g["data"], box, RES, cloud, guess, p)
        vol = P.scores()
        assert vol[0].tobytes() == vol[4].tobytes(), "the case must hold an exact tie"
        got = s.localize(1, est, cloud, guess, p)
        assert _winner(got) == P.brute(vol) and L.same_record(got, P.search())
        assert s.localize_scores(1, est, cloud, guess, p).tobytes() == vol.tobytes()
    s.close()


# ------------------------------------------------------------------ overflow
def test_overflow_is_unproven_and_repeatable(room_store):
    w = world()
    p = _params(half_x=40, half_y=40, half_a=15, angle_step=math.radians(1), coarse_shift=4, max_refine_blocks=1)
    guess = (QUERY_POSE[0] + 1.7, QUERY_POSE[1] - 2.2, QUERY_POSE[2] + 0.13)
    want = _problem(room_store, w.query, guess, p).search()
    a = room_store.localize(w.V, w.est, w.query, guess, p)
    b = room_store.localize(w.V, w.est, w.query, guess, p)
    assert int(a["status"]) == _abi.DPG_LOC_UNPROVEN and int(a["n_frontier"]) > 1
    assert L.same_record(a, want), (a, want)
    assert all(a[n].tobytes() == b[n].tobytes() for n in _abi.LOC_RESULT_EXACT)
    assert 31 <= int(a["n_refined_candidates"]) <= 31 * 256     # the seeds alone


# ------------------------------------------------------------------ recovery
RECOVERY = dict(half_a=180, angle_step=math.radians(1), coarse_shift=3)


def test_recovery_from_a_lost_guess(ctx, room_store):
    """The query scan with a guess 4 m and 100 degrees off, searched over the whole map (window="map")
    and the full circle at 1-degree steps; then ICP (downsample ratio 1, defaults otherwise) from the
    localised pose against the nearest node.
    Measured on the CPU, with loc_ref on the occupancy grid restated in numpy (occ_grid_ref over beam
    end points computed in numpy) and the CPU oracle's ICP:
      loc_ref's pruned search returns (6.4, 4.6, 1.106): 0.042 m and 0.000 degrees from the truth, score
        91100 of 91800, a frontier of 1 block of 532836;
      the oracle's ICP from that pose against node 4 ends 0.0080 m and 0.218 degrees from the truth;
      from the lost guess it ends 2.94 m and 86.8 degrees away.
    Here: the GPU record equals loc_ref's, and icp_batch_guess from it must end
    within test_end_to_end_guess_outside_icp_basin's bounds, 5 cm and 1 degree."""
    w = world()
    guess = (QUERY_POSE[0] - 3.2, QUERY_POSE[1] + 2.4, QUERY_POSE[2] + math.radians(100))    # 4 m, 100 degrees
    p = _params(**RECOVERY)
    r = room_store.localize(w.V, w.est, w.query, guess, p, window="map")
    gx, gy, hx, hy = room_store.map_window(w.V, w.est, p)
    _, box = _occ(room_store)
    assert 2 * hx + 1 >= box[2] and 2 * hy + 1 >= box[3]
    q = _params(half_x=hx, half_y=hy, **RECOVERY)
    want = _problem(room_store, w.query, (gx, gy, guess[2]), q).search()
    assert L.same_record(r, want), (r, want)
    assert int(r["status"]) == _abi.DPG_LOC_OK
    pose = r["pose"].astype(np.float64)
    d = [math.hypot(pose[0] - x, pose[1] - y) for x, y, _ in NODE_POSES]
    t = int(np.argmin(d))
    e_loc = (math.hypot(pose[0] - QUERY_POSE[0], pose[1] - QUERY_POSE[1]),
             abs(math.remainder(pose[2] - QUERY_POSE[2], 2 * math.pi)))
    with api.Context(0) as own:                       # a scan store of its own: the target node and the query
        pts = np.ascontiguousarray(np.concatenate([w.clouds[t], w.query]), f32)
        ip = _abi.default_icp_params()
        ip.downsample_icp_points_ratio = 1
        own.upload_scans(pts, np.array([0, NB, NB + len(w.query)], np.int64), 1)
        edges = np.array([[0, 1]], np.int32)
        g = api.icp_guess(r["pose"], w.est[t])[None, :]
        res, _ = own.icp_batch_guess(edges, g, ip, compute_cov=False)
    truth = api.inverse_transform_point(np.array(QUERY_POSE, f32), w.est[t])
    z = res["z"][0]
    e = (math.hypot(z[0] - truth[0], z[1] - truth[1]), abs(math.remainder(float(z[2]) - float(truth[2]), 2 * math.pi)))
    print(f"localised {pose} ({e_loc[0]:.4f} m, {math.degrees(e_loc[1]):.3f} deg off), score {int(r['score'])} of {255 * NB}, "
          f"frontier {int(r['n_frontier'])} of {int(r['n_blocks'])}; ICP against node {t}: {e[0]:.4f} m {math.degrees(e[1]):.3f} deg")
    assert res["converged"][0] and e[0] <= 0.05 and e[1] <= math.radians(1.0)


# ------------------------------------------------------------------ no side effects
def test_no_side_effects(ctx):
    """The change detection run twice over one workload, once with a localize call before every
    executeDPG: identical counters, node state, grids and map lists; a grid after a localize call
    equals one before it."""
    w = synth.make_dynamic(n_passes=2, nodes_per_pass=8, n_beams=NB, world_size=16.0, range_max=8.0, n_boxes=6, seed=9)
    a = api.DpgStore(ctx, w.ranges, w.geom)
    b = api.DpgStore(ctx, w.ranges, w.geom)
    n0 = int(w.pass_start[1])
    p = _params(half_x=20, half_y=20, half_a=10, angle_step=math.radians(2))
    for v in range(n0, w.V):
        cur = int(v - w.pass_start[w.pass_of[v]] + 1)
        est = w.est[:v + 1]
        cloud = api.scan_to_cloud(w.ranges[v], w.geom[v, 0], w.geom[v, 1], w.geom[v, 2])
        g1 = b.occupancy_grid(v + 1, est, counts=True)
        r = b.localize(v + 1, est, cloud, w.est[v], p)
        assert int(r["status"]) == _abi.DPG_LOC_OK
        g2 = b.occupancy_grid(v + 1, est, counts=True)
        ga = a.occupancy_grid(v + 1, est, counts=True)
        for k in ("hits", "misses", "data"):
            assert g1[k].tobytes() == g2[k].tobytes() == ga[k].tobytes(), (v, k)
        sa, sb = a.execute_dpg(v + 1, cur, est), b.execute_dpg(v + 1, cur, est)
        assert sa.counters() == sb.counters(), (v, sa.counters(), sb.counters())
        assert sa.grid_cells == sb.grid_cells and sa.n_samples == sb.n_samples, v
        for x, y in zip(a.fetch(), b.fetch()):
            assert np.array_equal(x, y), v
    la, lb = a.active_dynamic_points(w.V, w.est), b.active_dynamic_points(w.V, w.est)
    for k in la:
        assert np.array_equal(la[k], lb[k]), k
    a.close()
    b.close()


# ------------------------------------------------------------------ errors
def _raw_localize(store, est, cloud, n_pts, guess, p):
    r = _abi.LocResult()
    C.memset(C.byref(r), 0x5A, C.sizeof(r))
    e, c, g = np.ascontiguousarray(est, f32), np.ascontiguousarray(cloud, f32), np.ascontiguousarray(guess, f32)
    rc = lib().dpg_map_localize(store.handle, len(e), ptr(e, C.c_float), ptr(c, C.c_float), n_pts, ptr(g, C.c_float),
                                C.byref(p), C.byref(r))
    return rc, bytes(r)


def test_errors(ctx, room_store):
    w = world()
    s = room_store
    good = _params(half_x=6, half_y=5, half_a=1, coarse_shift=2)
    g = _guess_near_truth()
    untouched = bytes([0x5A]) * 128
    for bad in (_params(kernel_radius=8), _params(occupied_min=0), _params(coarse_shift=6), _params(half_a=1025),
                _params(max_refine_blocks=0), _params(sigma=0.0)):
        assert _raw_localize(s, w.est, w.query, len(w.query), g, bad) == (-1, untouched)
    assert _raw_localize(s, w.est, w.query, (1 << 23) + 1, g, good) == (-1, untouched)       # refused before the cloud is read
    assert _raw_localize(s, w.est, w.query, -1, g, good) == (-1, untouched)
    for bad_guess in ((1e12, 0.0, 0.0), (0.0, np.nan, 0.0), (0.0, 0.0, np.inf)):
        assert _raw_localize(s, w.est, w.query, len(w.query), bad_guess, good) == (-1, untouched)
    with pytest.raises(_abi.DpgError, match=r"\(-1\)"):
        s.localize(w.V + 1, np.zeros((w.V + 1, 3), f32), w.query, g, good)
    with pytest.raises(_abi.DpgError, match=r"\(-4\)"):                                       # the box above max_cells
        s.localize(w.V, w.est, w.query, g, _params(half_x=6, half_y=5, half_a=1, max_cells=64))
    with pytest.raises(_abi.DpgError, match=r"\(-4\)"):                                       # a bound volume above 2^29
        s.localize(w.V, w.est, w.query, g, _params(half_x=32768, half_y=32768, half_a=1024, coarse_shift=0))
    # capacities one short: DPG_ERR_SIZE and the sentinel bytes intact
    e, c, gg = w.est, w.query, np.array(g, f32)
    nb = 3 * 3 * 4
    out = np.full(nb, 0x5A5A5A5A, np.int32)
    args = (s.handle, w.V, ptr(e, C.c_float), ptr(c, C.c_float), len(c), ptr(gg, C.c_float), C.byref(good))
    assert lib().dpg_map_localize_bounds(*args, ptr(out, C.c_int32), nb - 1) == -4 and (out == 0x5A5A5A5A).all()
    assert lib().dpg_map_localize_bounds(*args, ptr(out, C.c_int32), nb) == 0 and not (out == 0x5A5A5A5A).any()
    nv = 3 * 11 * 13
    out = np.full(nv, 0x5A5A5A5A, np.int32)
    assert lib().dpg_map_localize_scores(*args, ptr(out, C.c_int32), nv - 1) == -4 and (out == 0x5A5A5A5A).all()
    assert lib().dpg_map_localize_scores(*args, ptr(out, C.c_int32), nv) == 0 and not (out == 0x5A5A5A5A).any()
    _, box = _occ(s)
    for shift, n in ((-1, box[2] * box[3]), (2, (box[2] + 3) * (box[3] + 3))):
        fb = np.full(n, 0x5A, np.uint8)
        bx = np.zeros(4, np.int32)
        assert lib().dpg_map_field(s.handle, w.V, ptr(e, C.c_float), C.byref(good), shift, ptr(fb, C.c_uint8), n - 1,
                                   ptr(bx, C.c_int32)) == -4 and (fb == 0x5A).all()
    with pytest.raises(_abi.DpgError, match=r"\(-1\)"):
        s.map_field(w.V, w.est, good, shift=6)
    with api.Context(0, virtual=2) as multi:                                                  # a multi-device form
        ms = world().store(multi)
        for call in (lambda: ms.localize(w.V, w.est, w.query, g, good), lambda: ms.map_field(w.V, w.est, good),
                     lambda: ms.localize_bounds(w.V, w.est, w.query, g, good),
                     lambda: ms.localize_scores(w.V, w.est, w.query, g, good)):
            with pytest.raises(_abi.DpgError, match=r"\(-3\)"):
                call()
        ms.close()


def test_buffers_regrow_between_calls(ctx):
    """A fresh store: a small request, a larger one (more points, angles and blocks, a pooled field),
    the small one again -- each equals the reference."""
    w = world()
    s = w.store(ctx)
    g = _guess_near_truth()
    small = _params(half_x=3, half_y=2, half_a=0, coarse_shift=0)
    large = _params(half_x=30, half_y=25, half_a=6, angle_step=math.radians(2), coarse_shift=2, max_refine_blocks=64)
    big_cloud = np.ascontiguousarray(np.concatenate([w.query, w.query + f32(0.03)]), f32)
    for cloud, p in ((w.query[:50], small), (big_cloud, large), (w.query[:50], small)):
        want = _problem(s, cloud, g, p).search()
        got = s.localize(w.V, w.est, cloud, g, p)
        assert L.same_record(got, want), (got, want)
    s.close()


# ------------------------------------------------------------------ through DpgSLAM
SLAM_WORLD = dict(n_passes=2, nodes_per_pass=8, n_beams=NB, world_size=16.0, range_max=8.0, n_boxes=6)
SLAM_SEED = 12
SLAM_LOC = dict(half_a=360, angle_step=math.radians(0.5), coarse_shift=3)


def _drive(slam, w):
    """Both passes through ObserveOdometry / ObserveLaser; returns the scan index of every node."""
    rng = np.random.default_rng(3)
    scan_of = []
    for ps in range(len(w.pass_start) - 1):
        if ps:
            slam.incrementPassNumber()
        for v in range(int(w.pass_start[ps]), int(w.pass_start[ps + 1])):
            odom = w.est[v].astype(np.float64) + rng.normal(0, [0.01, 0.01, 0.002])
            slam.ObserveOdometry(odom[:2].astype(f32), f32(odom[2]))
            slam.ObserveLaser(w.ranges[v], 0.0, float(w.geom[v, 2]), float(w.geom[v, 0]), float(w.geom[v, 1]))
            if len(slam.poses) > len(scan_of):
                scan_of.append(v)
    return scan_of


def _cross_pass_closures(F, n0, scan_of, w):
    """The cross-pass Between factors of a rebuilt graph, the successive pair (n0 - 1, n0) aside, as
    (i, j, metres, radians from the ground truth's relative pose)."""
    out = []
    for f in F[(F["kind"] == _abi.DPG_FACTOR_BETWEEN) & (F["i"] < n0) & (F["j"] >= n0)]:
        i, j = int(f["i"]), int(f["j"])
        if (i, j) == (n0 - 1, n0):
            continue
        t = api.inverse_transform_point(w.est[scan_of[j]], w.est[scan_of[i]])
        out.append((i, j, math.hypot(f["z"][0] - t[0], f["z"][1] - t[1]), abs(math.remainder(float(f["z"][2]) - float(t[2]), 2 * math.pi))))
    return out


def test_through_dpgslam():
    """Two passes of a synthetic world whose second pass starts 5.25 m from where the first began, at
    (4.797, 2.123, 0) in pass 0's frame (seed 12; seeds 1, 9, 10 and 23 also start elsewhere but their
    pass-0 maps are ambiguous under quarter turns, and 2 and 15 bring no pass-1 node within
    max_dist_across_passes of a pass-0 node).  Checked on the CPU before relying on it, with the CPU
    backend (tests/slam_oracle.py), loc_ref and an occupancy grid restated in numpy: the scan is
    localised at (4.8, 2.1, -1 degree), score 46298 of 81855, a frontier of 664 of 431158 blocks; after
    the sweep the node sits 0.007 m, 0.023 m and 0.87 degrees from the truth; the one cross-pass
    closure (3, 10) ends 0.010 m and 0.20 degrees from the truth, while all 18 closures of the run
    without the option are more than 5 m off.
    Without new_pass_start the pass-1 node is created at the origin of pass 0's frame and no cross-pass
    loop closure of the rebuilt graph agrees with the ground truth; with it the node is created at the
    localised pose, and that pose and the node's estimate after the sweep lie at the ground truth to
    within a cell and an angle step plus the ICP tolerance (5 cm, 1 degree), at least one cross-pass
    loop closure agrees with the ground truth to within the ICP tolerance, and the rebuilt graph's
    prior carries the localised mean."""
    from dpgslam.slam import DpgSLAM, GpuBackend

    class Recording(GpuBackend):
        def add_node(self, cloud, passes, init_pose, extra, *a):
            self.created = getattr(self, "created", []) + [(np.array(init_pose, f32), np.array(extra))]
            return super().add_node(cloud, passes, init_pose, extra, *a)

    w = synth.make_dynamic(seed=SLAM_SEED, **SLAM_WORLD)
    v0 = int(w.pass_start[1])
    truth = api.inverse_transform_point(w.est[v0], w.est[0])           # pass 1's start in pass 0's frame
    assert math.hypot(truth[0], truth[1]) > 2.0                        # beyond max_dist_across_passes
    lp = _abi.default_loc_params()
    lp.resolution = RES
    for k, v in SLAM_LOC.items():
        setattr(lp, k, v)
    runs = {}
    for name, kw in (("plain", {}), ("none", dict(new_pass_start=None)), ("on", dict(new_pass_start=lp, localize_min_response=0.3))):
        with api.Context(0) as c:
            be = Recording(c)
            s = DpgSLAM(backend=be, **kw)
            scan_of = _drive(s, w)
            n0 = scan_of.index(v0)
            s.incrementPassNumber()
            runs[name] = dict(factors=s.factors.tobytes(), poses=s.poses.tobytes(), F=s.factors.copy(), n0=n0,
                              created=be.created[n0], closures=_cross_pass_closures(s.factors, n0, scan_of, w),
                              loc=s.last_localization, start=dict(s.pass_start_pose), final=s.poses[n0].copy())
    assert runs["plain"]["factors"] == runs["none"]["factors"] and runs["plain"]["poses"] == runs["none"]["poses"]
    none, on = runs["none"], runs["on"]
    n0 = on["n0"]
    assert none["n0"] == n0 and none["loc"] is None and none["start"] == {}
    assert np.array_equal(none["created"][0], np.zeros(3, f32)) and np.array_equal(none["created"][1]["z"][0], np.zeros(3))
    r = on["loc"]
    assert r is not None and int(r["status"]) in (_abi.DPG_LOC_OK, _abi.DPG_LOC_UNPROVEN)
    assert np.array_equal(on["created"][0], r["pose"]) and np.array_equal(on["created"][1]["z"][0], r["pose"].astype(np.float64))

    def off(pose):
        return (abs(float(pose[0]) - truth[0]), abs(float(pose[1]) - truth[1]),
                abs(math.remainder(float(pose[2]) - float(truth[2]), 2 * math.pi)))
    e_loc, e_fin = off(r["pose"]), off(on["final"])
    tol = (0.05, math.radians(1.0))
    good = lambda cl: [c for c in cl if c[2] <= tol[0] and c[3] <= tol[1]]
    print(f"pass 1 starts at {truth} in pass 0's frame; localised {r['pose']} (off {e_loc[0]:.3f} {e_loc[1]:.3f} m "
          f"{math.degrees(e_loc[2]):.3f} deg) score {int(r['score'])} of {255 * int(r['n_pts'])}, status {int(r['status'])}, "
          f"frontier {int(r['n_frontier'])} of {int(r['n_blocks'])}; after the sweep off {e_fin[0]:.3f} {e_fin[1]:.3f} m "
          f"{math.degrees(e_fin[2]):.3f} deg; cross-pass closures at the truth: {len(good(none['closures']))} of "
          f"{len(none['closures'])} without, {len(good(on['closures']))} of {len(on['closures'])} with")
    for e in (e_loc, e_fin):
        assert e[0] <= RES + tol[0] and e[1] <= RES + tol[0] and e[2] <= SLAM_LOC["angle_step"] + tol[1], e
    assert len(good(none["closures"])) == 0 and len(good(on["closures"])) >= 1
    pri = on["F"][on["F"]["kind"] == _abi.DPG_FACTOR_PRIOR]
    assert list(pri["i"]) == [0, n0] and list(on["start"]) == [n0]
    assert np.array_equal(pri["z"][1], np.asarray(on["start"][n0], np.float64))
    assert np.array_equal(pri["z"][1].astype(f32), r["pose"]) and np.array_equal(pri["z"][0], np.zeros(3))
