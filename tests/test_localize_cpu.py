"""Localisation in the active map, the parts that need no GPU: the ABI structs and their defaults,
parameter validation, the host rotation table, the numpy restatement's pruned search against its own
brute force on synthetic byte grids (tests/loc_ref.py), and DpgSLAM's new_pass_start plumbing over a
fake backend."""
import ctypes as C
import math

import numpy as np
import pytest

import loc_ref as L
from dpgslam import _abi, api
from dpgslam._abi import lib, ptr
from dpgslam.slam import DpgSLAM

f32 = np.float32


def _params(**kw):
    p = _abi.default_loc_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_struct_sizes_and_defaults():
    assert C.sizeof(_abi.LocParams) == 56 and C.sizeof(_abi.LocResult) == 128 == _abi.LOC_RESULT_DTYPE.itemsize
    for name, _ in _abi.LocResult._fields_:
        assert getattr(_abi.LocResult, name).offset == _abi.LOC_RESULT_DTYPE.fields[name][1], name
    p = _abi.default_loc_params()
    assert (p.resolution, p.max_cells, p.margin_cells) == (0.0, 0, 1)
    assert (p.kernel_radius, p.occupied_min, p.half_x, p.half_y, p.half_a) == (3, 50, 40, 40, 360)
    assert (p.coarse_shift, p.max_refine_blocks) == (4, 16384)
    assert p.sigma == f32(0.1) and p.angle_step == f32(0.5 * math.pi / 180.0)
    assert (2 * p.half_a + 1) * p.angle_step > 2 * math.pi            # the default is the full circle
    assert api.loc_params_valid(p)
    assert (_abi.DPG_LOC_OK, _abi.DPG_LOC_NO_OVERLAP, _abi.DPG_LOC_UNPROVEN) == (0, 1, 2)


@pytest.mark.parametrize("field,good,bad", [
    ("resolution", (0.0, 0.05, 2.0), (-0.1, math.nan, math.inf)),
    ("max_cells", (0, 1, 1 << 25), (-1, (1 << 25) + 1)),
    ("margin_cells", (0, 7), (-1,)),
    ("sigma", (1e-3, 5.0), (0.0, -1.0, math.nan, math.inf)),
    ("kernel_radius", (0, 7), (-1, 8)),
    ("occupied_min", (1, 100), (0, -1, 101)),
    ("half_x", (0, 32768), (-1, 32769)),
    ("half_y", (0, 32768), (-1, 32769)),
    ("half_a", (0, 1024), (-1, 1025)),
    ("angle_step", (1e-4, 1.6), (0.0, -0.1, math.nan, math.inf)),
    ("coarse_shift", (0, 5), (-1, 6)),
    ("max_refine_blocks", (1, 1 << 30), (0, -5)),
])
def test_parameter_validation(field, good, bad):
    for v in good:
        assert api.loc_params_valid(_params(**{field: v})), (field, v)
    for v in bad:
        assert not api.loc_params_valid(_params(**{field: v})), (field, v)
        out = np.zeros((2 * 1024 + 1, 2), f32)
        assert lib().dpg_loc_rotations(0.0, C.byref(_params(**{field: v})), ptr(out, C.c_float)) == -1
    assert lib().dpg_loc_params_check(None) == -1


@pytest.mark.parametrize("theta,half_a,step", [(0.0, 0, 0.1), (0.3, 7, math.radians(0.5)), (-2.9, 360, math.radians(0.5)),
                                               (1.0, 1024, math.radians(0.25))])
def test_rotations_against_numpy(theta, half_a, step):
    p = _params(half_a=half_a, angle_step=step)
    rot = api.loc_rotations(theta, p)
    ang = np.float64(f32(theta)) + (np.arange(2 * half_a + 1) - half_a).astype(np.float64) * np.float64(f32(step))
    assert rot.shape == (2 * half_a + 1, 2) and rot.dtype == f32
    # libm against numpy: the same double function up to its last bit, then one rounding to float
    np.testing.assert_allclose(rot[:, 0], np.cos(ang), rtol=0, atol=6e-8)
    np.testing.assert_allclose(rot[:, 1], np.sin(ang), rtol=0, atol=6e-8)
    np.testing.assert_array_equal(rot[half_a], [f32(math.cos(float(f32(theta)))), f32(math.sin(float(f32(theta))))])


# ------------------------------------------------------------------ the restatement against itself
def _room_grid(w=70, h=60, square=False):
    """Occupancy bytes of a walled room with a box, and the cloud of its occupied cells seen from a
    pose inside it (res 0.1)."""
    occ = np.full((h, w), -1, np.int8)
    x1, y1 = (w - 11, h - 11) if not square else (min(w, h) - 11, min(w, h) - 11)
    occ[11:y1, 11:x1] = 0
    occ[10, 10:x1 + 1] = 100
    occ[y1, 10:x1 + 1] = 100
    occ[10:y1 + 1, 10] = 100
    occ[10:y1 + 1, x1] = 100
    if not square:
        occ[30:35, 30] = 80
        occ[22, 40:47] = 49        # below the default threshold: never in the field
    return occ


def _cloud_of(occ, box, res, pose, thr=50):
    ys, xs = np.nonzero(occ >= thr)
    wx, wy = (xs + box[0]) * res - pose[0], (ys + box[1]) * res - pose[1]
    c, s = math.cos(-pose[2]), math.sin(-pose[2])
    return np.stack([c * wx - s * wy, s * wx + c * wy], 1).astype(f32)


def _agree(P):
    """The pruned search's record names the brute-force winner; bound >= every score of its block."""
    vol, bvol = P.scores(), P.bounds()
    r = P.search(bvol)
    assert P.brute(vol) == (int(r["score"]), int(r["best_a"]), int(r["best_dx"]), int(r["best_dy"]))
    for a in range(P.A):
        for by in range(P.nby):
            for bx in range(P.nbx):
                sc, dx0, dy0 = P.block_scores(a, bx, by)
                assert np.array_equal(sc, vol[a, dy0 + P.hy:dy0 + P.hy + sc.shape[0], dx0 + P.hx:dx0 + P.hx + sc.shape[1]])
                assert bvol[a, by, bx] >= sc.max(), (a, by, bx)
    assert int(r["score_at_guess"]) == int(vol[P.ha, P.hy, P.hx])
    return r, vol


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("hx,hy", [(10, 0), (13, 9), (0, 5), (8, 8)])   # 2 h + 1 = 21, 27, 19, 1, 11, 17: never a multiple of 2, 4, 8
def test_pruned_search_equals_brute_force(shift, hx, hy):
    occ, box, res = _room_grid(), (-5, -7, 70, 60), 0.1
    cloud = _cloud_of(occ, box, res, (3.0, 2.3, 0.4))
    p = _params(half_x=hx, half_y=hy, half_a=6, angle_step=math.radians(5), coarse_shift=shift)
    r, _ = _agree(L.Problem(occ, box, res, cloud, (2.5, 2.0, 0.2), p))
    assert int(r["status"]) == _abi.DPG_LOC_OK and int(r["n_frontier"]) >= 1
    assert int(r["n_blocks"]) == 13 * (-(-(2 * hx + 1) // (1 << shift))) * (-(-(2 * hy + 1) // (1 << shift)))


def test_pruned_search_keeps_the_tie_order():
    """A square room seen from its centre, the full circle at 90-degree steps: the four quarter
    turns and the two half turns (a = 0 and a = 4 are the same rotation) tie exactly."""
    occ, box, res = _room_grid(61, 61, square=True), (-30, -30, 61, 61), 0.1
    cloud = _cloud_of(occ, box, res, (0.0, 0.0, 0.0))
    for shift in (0, 2, 3):
        p = _params(half_x=6, half_y=6, half_a=2, angle_step=math.pi / 2, coarse_shift=shift)
        P = L.Problem(occ, box, res, cloud, (0.0, 0.0, 0.0), p)
        r, vol = _agree(P)
        assert (vol == vol.max()).sum() >= 4, "the case must hold an exact tie"
        assert (int(r["best_a"]), int(r["best_dx"]), int(r["best_dy"])) == (2, 0, 0)   # the smallest |a - ha| of the tied
        # off-centre guess: the tie between a = 0 and a = 4 (|a - ha| = 2 both) goes to the smaller a
        p2 = _params(half_x=6, half_y=6, half_a=2, angle_step=math.pi / 2, coarse_shift=shift)
        P2 = L.Problem(occ, box, res, cloud, (0.2, -0.1, math.pi), p2)
        r2, vol2 = _agree(P2)
        assert vol2[0].max() == vol2[4].max() == vol2.max() and int(r2["best_a"]) in (0, 2)


def test_overflow_and_no_overlap_statuses():
    occ, box, res = _room_grid(), (-5, -7, 70, 60), 0.1
    cloud = _cloud_of(occ, box, res, (3.0, 2.3, 0.4))
    p = _params(half_x=13, half_y=9, half_a=6, angle_step=math.radians(5), coarse_shift=3, max_refine_blocks=1)
    P = L.Problem(occ, box, res, cloud, (2.5, 2.0, 0.2), p)
    r = P.search()
    assert int(r["status"]) == _abi.DPG_LOC_UNPROVEN and int(r["n_frontier"]) > 1
    assert int(r["n_refined_candidates"]) <= 13 * 64 and int(r["score"]) <= P.brute()[0]
    far = L.Problem(occ, box, res, cloud, (500.0, 2.0, 0.2), p).search()     # the window wholly outside the box
    assert int(far["status"]) == _abi.DPG_LOC_NO_OVERLAP and int(far["score"]) == 0
    assert (int(far["best_a"]), int(far["best_dx"]), int(far["best_dy"])) == (6, 0, 0)
    none = L.Problem(np.zeros((0, 0), np.int8), (0, 0, 0, 0), res, cloud, (0, 0, 0), p).search()   # no active node
    assert int(none["status"]) == _abi.DPG_LOC_NO_OVERLAP and int(none["n_frontier"]) == 0


def test_field_and_pool_on_a_single_cell():
    occ = np.full((9, 11), -1, np.int8)
    occ[4, 5] = 50
    p = _params(kernel_radius=2, sigma=0.1)
    F = L.field(occ, p, 0.1)
    lut = L.lut_of(p, 0.1)
    assert F[4, 5] == 255 == lut[0] and F[4, 7] == lut[4] and F[6, 6] == 0 and F[5, 6] == lut[2] and F.sum() == sum(
        int(lut[ox * ox + oy * oy]) for ox in range(-2, 3) for oy in range(-2, 3) if ox * ox + oy * oy <= 4)
    assert not L.field(occ, _params(kernel_radius=2, occupied_min=51), 0.1).any()
    P = L.pooled(F, 2)
    assert P.shape == (12, 14)
    for y in range(-3, 9):
        for x in range(-3, 11):
            blk = F[max(y, 0):max(y + 4, 0), max(x, 0):max(x + 4, 0)]
            assert P[y + 3, x + 3] == (blk.max() if blk.size else 0)
    assert np.array_equal(L.pooled(F, 0), F)


# ------------------------------------------------------------------ DpgSLAM over a fake backend
ICP_DTYPE = np.dtype([("converged", "<i4"), ("status", "<i4"), ("z", "<f4", (3,))])


class FakeStore:
    def __init__(self, record):
        self.record, self.calls = record, []

    def append(self, *a):
        pass

    def execute_dpg(self, n_nodes, cur, est, chain_poses=None):
        return None

    def localize(self, n_nodes, est, cloud, guess=(0.0, 0.0, 0.0), params=None, window=None):
        self.calls.append((n_nodes, np.array(est), np.array(cloud), tuple(guess), params, window))
        return self.record


class StoreWithout(FakeStore):
    localize = None


class FakeBackend:
    """Keeps every node where it was created and records the factors it is handed."""

    def __init__(self, store):
        self._store, self.init, self.extras, self.rebuilt = store, [], [], None

    def add_node(self, cloud, passes, init_pose, extra, icp_params, reopt_params, non_successive):
        self.init.append(np.array(init_pose, np.float64))
        self.extras.append(np.array(extra))
        return 0, np.array(self.init)

    def candidates(self, est, passes, within, across):
        return np.zeros((0, 2), np.int32)

    def icp_batch(self, clouds, edges, est, p):
        r = np.zeros(len(edges), ICP_DTYPE)
        r["converged"] = 1
        return r

    def rebuild_graph(self, est, F):
        self.rebuilt = np.array(F)
        return est

    def store(self, ranges, geom, offsets, params):
        return self._store


def _record(pose=(3.5, -1.25, 0.75), score=40000, n_pts=360, status=_abi.DPG_LOC_OK):
    r = np.zeros((), _abi.LOC_RESULT_DTYPE)
    r["pose"], r["score"], r["n_pts"], r["status"] = pose, score, n_pts, status
    return r


def _two_passes(slam):
    """Pass 0 of two nodes, then the first scan of pass 1 and one more node."""
    scan = np.full(360, 4.0, f32)
    for pss in range(2):
        if pss:
            slam.incrementPassNumber()
        for k in range(2):
            slam.ObserveOdometry(np.array([1.5 * k, 0.0], f32), f32(0.0))
            slam.ObserveLaser(scan, 0.0, 10.0, -math.pi, math.pi)
    return scan


def _priors(F):
    F = np.asarray(F).reshape(-1)
    return F[F["kind"] == _abi.DPG_FACTOR_PRIOR]


@pytest.mark.parametrize("status", [_abi.DPG_LOC_OK, _abi.DPG_LOC_UNPROVEN])
def test_slam_starts_a_pass_at_the_localised_pose(status):
    lp = _params(half_a=90, angle_step=math.radians(2))
    store = FakeStore(_record(status=status))
    be = FakeBackend(store)
    slam = DpgSLAM(backend=be, new_pass_start=lp, localize_min_response=0.3)
    scan = _two_passes(slam)
    pose = np.array([3.5, -1.25, 0.75], f32)
    # one attempt, for the first scan of pass 1, over the two nodes of pass 0, whole map, the caller's params
    assert len(store.calls) == 1
    n_nodes, est, cloud, guess, params, window = store.calls[0]
    assert n_nodes == 2 and est.shape == (2, 3) and window == "map" and params is lp
    assert np.array_equal(cloud, api.scan_to_cloud(scan, f32(-math.pi), f32(math.pi), f32(10.0), slam.laser))
    assert slam.last_localization is store.record
    # the node, the prior handed to the graph, and the prior of the rebuilt graph
    assert np.array_equal(be.init[2].astype(f32), pose) and np.array_equal(slam.poses[2], pose)
    assert be.extras[2]["kind"][0] == _abi.DPG_FACTOR_PRIOR and be.extras[2]["i"][0] == 2
    assert np.array_equal(be.extras[2]["z"][0], pose.astype(np.float64))
    assert np.array_equal(be.extras[0]["z"][0], np.zeros(3))
    # the next node of the pass hangs off the localised one by odometry
    assert abs(float(slam.poses[3][0]) - (3.5 + 1.5 * math.cos(0.75))) < 1e-5
    slam.incrementPassNumber()
    pri = _priors(slam.factors)
    assert list(pri["i"]) == [0, 2]
    assert np.array_equal(pri["z"][0], np.zeros(3)) and np.array_equal(pri["z"][1], pose.astype(np.float64))
    assert np.array_equal(pri["info"][1], api.prior_factor(2)["info"][0])
    assert np.array_equal(_priors(be.rebuilt)["z"], pri["z"])


@pytest.mark.parametrize("record", [_record(score=int(0.29 * 255 * 360)), _record(status=_abi.DPG_LOC_NO_OVERLAP)])
def test_slam_falls_back_to_the_origin(record):
    store = FakeStore(record)
    be = FakeBackend(store)
    slam = DpgSLAM(backend=be, new_pass_start=_params(), localize_min_response=0.3)
    _two_passes(slam)
    assert len(store.calls) == 1 and slam.last_localization is record and slam.pass_start_pose == {}
    assert np.array_equal(be.init[2], np.zeros(3)) and np.array_equal(be.extras[2]["z"][0], np.zeros(3))
    slam.incrementPassNumber()
    assert np.array_equal(_priors(slam.factors)["z"], np.zeros((2, 3)))


def test_slam_without_the_option_never_localises():
    off, on = FakeStore(_record()), FakeStore(_record(status=_abi.DPG_LOC_NO_OVERLAP))
    runs = []
    for store, kw in ((off, {}), (off, dict(new_pass_start=None)), (on, dict(new_pass_start=_params()))):
        be = FakeBackend(store)
        slam = DpgSLAM(backend=be, **kw)
        _two_passes(slam)
        slam.incrementPassNumber()
        runs.append((slam.factors.tobytes(), slam.poses.tobytes(), [e.tobytes() for e in be.extras]))
    assert off.calls == [] and len(on.calls) == 1
    assert runs[0] == runs[1] == runs[2]        # a refused localisation leaves the reference's behaviour


def test_slam_needs_the_method():
    slam = DpgSLAM(backend=FakeBackend(StoreWithout(None)), new_pass_start=_params())
    with pytest.raises(NotImplementedError, match=r"Localize needs a `localize\(.*\)` method on the backend's node store; "
                                                  r"StoreWithout has none"):
        _two_passes(slam)
    plain = DpgSLAM(backend=FakeBackend(StoreWithout(None)))
    with pytest.raises(ValueError, match="no node yet"):
        plain.Localize(np.full(8, 1.0, f32), 10.0, -1.0, 1.0)
    _two_passes(plain)                          # without the option the store is never asked
    with pytest.raises(NotImplementedError):
        plain.Localize(np.full(8, 1.0, f32), 10.0, -1.0, 1.0)
