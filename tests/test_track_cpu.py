"""The frozen map and the tracker without a GPU: the ABI structs, the host checks (track params, the
map file's header), the numpy restatement tests/track_ref.py against its own brute force, and
DpgSLAM's localisation-only mode over a fake store and backend."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import track_ref as T
from dpgslam import _abi, api
from dpgslam._abi import lib
from dpgslam.slam import DpgSLAM

f32 = np.float32


# ------------------------------------------------------------------ ABI
def test_struct_sizes_and_defaults():
    assert C.sizeof(_abi.TrackParams) == 16 and C.sizeof(_abi.TrackResult) == 48 and C.sizeof(_abi.FmapInfo) == 48
    assert [(n, getattr(_abi.TrackParams, n).offset) for n, _ in _abi.TrackParams._fields_] == \
        [("half_x", 0), ("half_y", 4), ("half_a", 8), ("angle_step", 12)]
    offs = {n: getattr(_abi.TrackResult, n).offset for n, _ in _abi.TrackResult._fields_}
    assert offs == dict(pose=0, rot=12, score=20, score_at_guess=24, n_pts=28, best_a=32, best_dx=36, best_dy=40, status=44)
    assert {n: _abi.TRACK_RESULT_DTYPE.fields[n][1] for n in _abi.TRACK_RESULT_DTYPE.names} == offs
    info = {n: getattr(_abi.FmapInfo, n).offset for n, _ in _abi.FmapInfo._fields_}
    assert info == dict(box=0, res=16, sigma=24, kernel_radius=28, occupied_min=32, pad=36, n_bytes=40)
    p = _abi.default_track_params()
    assert (p.half_x, p.half_y, p.half_a) == (10, 10, 10) and p.angle_step == f32(math.radians(0.5))
    assert lib().dpg_track_params_check(C.byref(p)) == 0
    assert lib().dpg_track_params_check(None) == -1


@pytest.mark.parametrize("field,good,bad", [
    ("half_x", (0, 64), (-1, 65)), ("half_y", (0, 64), (-1, 65)), ("half_a", (0, 64), (-1, 65)),
    ("angle_step", (1e-6, 3.0), (0.0, -0.1, float("nan"), float("inf"))),
])
def test_track_params_check(field, good, bad):
    for v in good:
        p = _abi.default_track_params()
        setattr(p, field, v)
        assert lib().dpg_track_params_check(C.byref(p)) == 0, (field, v)
    for v in bad:
        p = _abi.default_track_params()
        setattr(p, field, v)
        assert lib().dpg_track_params_check(C.byref(p)) == -1, (field, v)


# ------------------------------------------------------------------ the file header
def _header(magic=b"DPGFMAP1", version=1, kr=3, om=50, sigma=0.1, res=0.1, box=(-5, -7, 70, 60), n_bytes=None, reserved=bytes(8)):
    n = box[2] * box[3] if n_bytes is None else n_bytes
    h = magic + struct.pack("<Iiifd4iq", version, kr, om, sigma, res, *box, n) + reserved
    assert len(h) == 64
    return h


def _check(h, size):
    buf = C.create_string_buffer(h, 64)
    return lib().dpg_fmap_header_check(C.cast(buf, C.c_void_p), size)


def test_fmap_header_check():
    good = _header()
    assert _check(good, 64 + 4200) == 0
    assert _check(_header(box=(0, 0, 0, 0)), 64) == 0                           # an empty map
    assert _check(_header(box=(3, 4, 8192, 4096)), 64 + (1 << 25)) == 0         # the ceiling
    assert _check(_header(kr=-9, om=1000, sigma=float("nan")), 64 + 4200) == 0  # metadata is not judged
    assert _check(good, 64 + 4199) == -1 and _check(good, 64 + 4201) == -1      # a short and a long file
    assert _check(good, 63) == -1
    for bad in (_header(magic=b"DPGFMAP2"), _header(magic=b"dpgfmap1"), _header(version=0), _header(version=2),
                _header(res=0.0), _header(res=-0.1), _header(res=float("nan")), _header(res=float("inf")),
                _header(box=(-5, -7, -70, -60), n_bytes=4200), _header(box=(-5, -7, -1, 60), n_bytes=4200),
                _header(box=(-5, -7, 70, -1), n_bytes=4200), _header(n_bytes=4199), _header(n_bytes=-4200),
                _header(reserved=b"\0" * 7 + b"\1"), _header(reserved=b"\1" + b"\0" * 7)):
        assert _check(bad, 64 + 4200) == -1, bad
    assert _check(_header(box=(0, 0, 8192, 4097)), 64 + 8192 * 4097) == -1      # above 2^25 cells
    assert lib().dpg_fmap_header_check(None, 64) == -1


# ------------------------------------------------------------------ the restatement against its own brute force
def _room_field(w=70, h=60, square=False):
    """A byte grid shaped like a likelihood field: walls of 255 with a one-cell halo of 120, a box."""
    F = np.zeros((h, w), np.uint8)
    x1, y1 = (w - 11, h - 11) if not square else (min(w, h) - 11, min(w, h) - 11)

    def wall(ys, xs, v):
        F[ys, xs] = np.maximum(F[ys, xs], v)
    for v, d in ((120, 1), (255, 0)):
        for o in range(-d, d + 1):
            wall(10 + o, slice(10, x1 + 1), v)
            wall(y1 + o, slice(10, x1 + 1), v)
            wall(slice(10, y1 + 1), 10 + o, v)
            wall(slice(10, y1 + 1), x1 + o, v)
            if not square:
                wall(slice(30, 35), 30 + o, v)
    return F


def _cloud_of(F, box, res, pose):
    ys, xs = np.nonzero(F == 255)
    wx, wy = (xs + box[0]) * res - pose[0], (ys + box[1]) * res - pose[1]
    c, s = math.cos(-pose[2]), math.sin(-pose[2])
    return np.stack([c * wx - s * wy, s * wx + c * wy], 1).astype(f32)


def _brute(P):
    """Every candidate scored point by point in Python integers, the winner by a plain sort."""
    h, w = P.F.shape if not P.empty else (0, 0)
    best, at_guess = None, None
    for a in range(P.A):
        kx, ky = T.L.point_keys(P.cloud, P.rot[a], P.res)
        for dy in range(-P.hy, P.hy + 1):
            for dx in range(-P.hx, P.hx + 1):
                x, y = kx + P.cx + dx - P.box[0], ky + P.cy + dy - P.box[1]
                ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
                sc = int(P.F[y[ok], x[ok]].astype(np.int64).sum()) if ok.any() else 0
                key = (-sc, abs(a - P.ha), dx * dx + dy * dy, a, dy, dx)
                best = key if best is None or key < best else best
                if (a, dx, dy) == (P.ha, 0, 0):
                    at_guess = sc
    return (-best[0], best[3], best[5], best[4]), at_guess


@pytest.mark.parametrize("hx,hy,ha", [(0, 0, 0), (1, 1, 0), (4, 2, 3), (0, 5, 1)])
def test_track_ref_equals_its_brute_force(hx, hy, ha):
    F, box, res = _room_field(), (-5, -7, 70, 60), 0.1
    cloud = _cloud_of(F, box, res, (3.0, 2.3, 0.4))
    cloud[5] = [np.nan, 0.0]
    tp = T.track_params(hx, hy, ha, math.radians(2))
    P = T.Problem(F, box, res, cloud, (2.9, 2.2, 0.43), tp)
    r = P.track_record()
    win, at_guess = _brute(P)
    assert (int(r["score"]), int(r["best_a"]), int(r["best_dx"]), int(r["best_dy"])) == win
    assert int(r["score_at_guess"]) == at_guess and int(r["n_pts"]) == len(cloud) and int(r["status"]) == _abi.DPG_LOC_OK
    assert r["pose"][0] == f32(np.float64(P.cx + win[2]) * 0.1) and r["pose"][1] == f32(np.float64(P.cy + win[3]) * 0.1)
    assert r["pose"][2] == f32(np.float64(f32(0.43)) + (win[1] - ha) * np.float64(f32(math.radians(2))))
    assert np.array_equal(r["rot"], P.rot[win[1]])


def test_track_ref_off_the_map_and_empty():
    F, box = _room_field(), (-5, -7, 70, 60)
    cloud = _cloud_of(F, box, 0.1, (3.0, 2.3, 0.4))
    tp = T.track_params(3, 2, 1)
    for P in (T.Problem(F, box, 0.1, cloud, (500.0, -300.0, 0.1), tp), T.Problem(np.zeros(0, np.uint8), (0, 0, 0, 0), 0.1, cloud, (1.0, 2.0, 0.1), tp),
              T.Problem(F, box, 0.1, cloud[:0], (3.0, 2.3, 0.4), tp)):
        r = P.track_record()
        assert (int(r["score"]), int(r["best_a"]), int(r["best_dx"]), int(r["best_dy"])) == (0, 1, 0, 0) == _brute(P)[0]
        assert int(r["status"]) == _abi.DPG_LOC_NO_OVERLAP and int(r["score_at_guess"]) == 0
        assert r["pose"][0] == f32(np.float64(P.cx) * 0.1) and r["pose"][2] == P.guess[2]


def test_track_ref_keeps_the_tie_order():
    """A square room seen from its centre, the full circle at 90-degree steps: the quarter turns tie."""
    F, box = _room_field(61, 61, square=True), (-30, -30, 61, 61)
    cloud = _cloud_of(F, box, 0.1, (0.0, 0.0, 0.0))
    P = T.Problem(F, box, 0.1, cloud, (0.0, 0.0, 0.0), T.track_params(3, 3, 2, math.pi / 2))
    vol = P.scores()
    assert (vol == vol.max()).sum() >= 4, "the case must hold an exact tie"
    r = P.track_record(vol)
    assert (int(r["best_a"]), int(r["best_dx"]), int(r["best_dy"])) == (2, 0, 0) == _brute(P)[0][1:]
    P2 = T.Problem(F, box, 0.1, cloud, (0.2, -0.1, math.pi), T.track_params(3, 3, 2, math.pi / 2))
    r2 = P2.track_record()
    assert (int(r2["score"]), int(r2["best_a"]), int(r2["best_dx"]), int(r2["best_dy"])) == _brute(P2)[0]


# ------------------------------------------------------------------ DpgSLAM's mode over fakes
ICP_DTYPE = _abi.RESULT_DTYPE


class FakeMap:
    def __init__(self, records):
        self.records, self.calls, self.closed = list(records), [], False

    def track(self, clouds, guesses, params=None):
        self.calls.append((np.array(clouds[0]), np.array(guesses[0], f32), params))
        return np.array([self.records.pop(0)])

    def close(self):
        self.closed = True


class FakeStore:
    def __init__(self, fmap=None):
        self.fmap, self.frozen, self.appended = fmap, [], 0

    def append(self, *a):
        self.appended += 1

    def execute_dpg(self, n_nodes, cur, est, chain_poses=None):
        return None

    def freeze(self, n_nodes, est, params=None):
        self.frozen.append((n_nodes, np.array(est), params))
        return self.fmap


class StoreWithout(FakeStore):
    freeze = None


class FakeBackend:
    def __init__(self, store):
        self._store, self.init, self.extras = store, [], []

    def add_node(self, cloud, passes, init_pose, extra, icp_params, reopt_params, non_successive):
        self.init.append(np.array(init_pose, np.float64))
        self.extras.append(np.array(extra))
        return 0, np.array(self.init)

    def store(self, ranges, geom, offsets, params):
        return self._store


def _rec(pose=(0.0, 0.0, 0.0), score=60000, n_pts=360, status=_abi.DPG_LOC_OK):
    r = np.zeros((), _abi.TRACK_RESULT_DTYPE)
    r["pose"], r["score"], r["n_pts"], r["status"] = pose, score, n_pts, status
    return r


SCAN = np.full(360, 4.0, f32)


def _map_two_nodes(slam):
    for k in range(2):
        slam.ObserveOdometry(np.array([1.5 * k, 0.0], f32), f32(0.0))
        slam.ObserveLaser(SCAN, 0.0, 10.0, -math.pi, math.pi)
    assert len(slam.poses) == 2


def _state(slam, be):
    return (slam.poses.tobytes(), slam.n_factors, len(be.init), [e.tobytes() for e in be.extras], slam.odom_at_last_align.tobytes(),
            slam.node_pass.tobytes(), len(slam.clouds), list(slam.current_pass))


def test_slam_mode_tracks_and_creates_nothing():
    good, weak, lost = _rec((2.0, 0.5, 0.1)), _rec((9.0, 9.0, 1.0), score=int(0.29 * 255 * 360)), _rec(status=_abi.DPG_LOC_NO_OVERLAP, score=0)
    fmap = FakeMap([good, weak, lost, _rec((4.0, 0.0, 0.0))])
    store = FakeStore(fmap)
    be = FakeBackend(store)
    slam = DpgSLAM(backend=be)
    _map_two_nodes(slam)
    lp, tp = _abi.default_loc_params(), _abi.default_track_params()
    before = _state(slam, be)
    slam.StartLocalization(track_params=tp, loc_params=lp, min_response=0.3, icp_refine=False)
    assert len(store.frozen) == 1 and store.frozen[0][0] == 2 and store.frozen[0][2] is lp
    assert np.array_equal(store.frozen[0][1], slam.poses)
    loc, ang = slam.GetPose()
    assert np.array_equal(loc, slam.poses[1][:2]) and ang == slam.poses[1][2]
    # 1: a good track.  The guess is the last node's estimate plus the odometry since the mode began.
    slam.ObserveOdometry(np.array([2.0, 0.25], f32), f32(0.05))
    slam.ObserveLaser(SCAN, 0.0, 10.0, -math.pi, math.pi)
    cloud, guess, params = fmap.calls[0]
    assert params is tp and np.array_equal(cloud, api.scan_to_cloud(SCAN, f32(-math.pi), f32(math.pi), f32(10.0), slam.laser))
    assert np.allclose(guess, [slam.poses[1][0] + 0.5, slam.poses[1][1] + 0.25, 0.05], atol=1e-6)
    assert slam.last_track is not None and np.array_equal(slam.last_track["pose"], good["pose"])
    loc, ang = slam.GetPose()
    assert np.array_equal(loc, f32([2.0, 0.5])) and ang == f32(0.1)          # the tracked pose, no odometry since
    # 2: a weak response is refused: the pose dead-reckons from the last accepted track
    slam.ObserveOdometry(np.array([3.0, 0.25], f32), f32(0.05))
    slam.ObserveLaser(SCAN, 0.0, 10.0, -math.pi, math.pi)
    g2 = fmap.calls[1][1]
    want = api.transform_point(api.inverse_transform_point(f32([3.0, 0.25, 0.05]), f32([2.0, 0.25, 0.05])), f32([2.0, 0.5, 0.1]))
    assert np.allclose(g2, want, atol=1e-5) and np.array_equal(slam.last_track["pose"], weak["pose"])
    loc, ang = slam.GetPose()
    assert np.allclose([loc[0], loc[1], ang], want, atol=1e-5)
    # 3: NO_OVERLAP is refused as well, and the odometry keeps accumulating from the same track
    slam.ObserveOdometry(np.array([4.0, 0.25], f32), f32(0.05))
    slam.ObserveLaser(SCAN, 0.0, 10.0, -math.pi, math.pi)
    want = api.transform_point(api.inverse_transform_point(f32([4.0, 0.25, 0.05]), f32([2.0, 0.25, 0.05])), f32([2.0, 0.5, 0.1]))
    assert np.allclose(fmap.calls[2][1], want, atol=1e-5)
    # 4: accepted again
    slam.ObserveLaser(SCAN, 0.0, 10.0, -math.pi, math.pi)
    assert np.array_equal(slam.GetPose()[0], f32([4.0, 0.0]))
    # nothing was created, and leaving the mode changes nothing else
    slam.StopLocalization()
    assert fmap.closed and _state(slam, be) == before and len(fmap.calls) == 4
    loc, ang = slam.GetPose()                                               # mapping's GetPose again: node 1 plus the odometry
    assert np.allclose(loc, [slam.poses[1][0] + 2.5, slam.poses[1][1] + 0.25], atol=1e-5)
    slam.ObserveLaser(SCAN, 0.0, 10.0, -math.pi, math.pi)                   # the next scan makes a node as usual
    assert len(slam.poses) == 3 and len(fmap.calls) == 4


def test_slam_mode_on_a_given_map_without_nodes():
    fmap = FakeMap([_rec((1.0, 2.0, 0.3))])
    slam = DpgSLAM(backend=FakeBackend(FakeStore()))
    with pytest.raises(ValueError, match="no node yet"):
        slam.StartLocalization(icp_refine=False)
    slam.StartLocalization(fmap=fmap, pose=(1.1, 2.1, 0.25), icp_refine=False)
    loc, ang = slam.GetPose()
    assert np.array_equal(loc, f32([1.1, 2.1])) and ang == f32(0.25)
    slam.ObserveLaser(SCAN, 0.0, 10.0, -math.pi, math.pi)                   # no odometry yet: the guess is the pose
    assert np.array_equal(fmap.calls[0][1], f32([1.1, 2.1, 0.25])) and fmap.calls[0][2] is None
    assert np.array_equal(slam.GetPose()[0], f32([1.0, 2.0])) and len(slam.poses) == 0
    slam.StopLocalization()
    assert not fmap.closed                                                  # the caller's map stays open


def test_slam_mode_needs_the_methods():
    slam = DpgSLAM(backend=FakeBackend(StoreWithout()))
    _map_two_nodes(slam)
    with pytest.raises(NotImplementedError, match=r"StartLocalization needs a `freeze\(.*\)` method on the backend's node store; "
                                                  r"StoreWithout has none"):
        slam.StartLocalization(icp_refine=False)
    with pytest.raises(NotImplementedError, match=r"needs a `track\(.*\)` method on the map; object has none"):
        slam.StartLocalization(fmap=object(), icp_refine=False)
    with pytest.raises(NotImplementedError, match=r"needs a `ctx.run_icp` on the backend; FakeBackend has none"):
        slam.StartLocalization(fmap=FakeMap([]))
