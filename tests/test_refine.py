"""The field refinement (dpg_fmap_refine, _trace, dpg_fmap_track_refine) on the GPU, byte for byte
against the numpy restatement tests/refine_ref.py: every fp64 operation is one rounding on both sides
and the summation order is fixed by the contract, so no tolerance is needed or allowed.  Where a byte
differs, the trace names the evaluation and the sum.

World: test_track.py's -- csm_ref's 12 x 9 m room scanned from six poses into a DpgStore, frozen at a
resolution of 0.1 m."""
import ctypes as C
import math

import numpy as np
import pytest

import refine_ref as R
import track_ref as T
from test_refine_cpu import START_OFFSETS, _corridor, _corridor_cloud, check_accuracy, grid_start
from test_track import AMAX, AMIN, GUESS, QUERY_POSE, RES, RMAX, _cloud_at, _cloud_of_size, _lp, world
from dpgslam import _abi, api
from dpgslam._abi import lib, ptr
from dpgslam.slam import DpgSLAM

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
KCHUNK = 2048     # points of a scan that the kernel keeps in LDS
NAMES = _abi.REFINE_RESULT_DTYPE.names


@pytest.fixture(scope="module")
def room(ctx):
    """(frozen map, F, box): computed once and left unchanged."""
    w = world()
    s = w.store(ctx)
    m = s.freeze(w.V, w.est, _lp())
    s.close()
    yield m, m.field(), m.info()["box"]
    m.close()


def _explain(got, want, g_tr=None, w_tr=None):
    """Where two sets of records (and traces) differ: scan, field; scan, evaluation, column."""
    msg = []
    for b in range(len(got)):
        msg += [f"scan {b} {n}: {got[b][n]} != {want[b][n]}" for n in NAMES if got[b][n].tobytes() != want[b][n].tobytes()]
    if g_tr is not None and g_tr.tobytes() != w_tr.tobytes():
        d = np.argwhere(g_tr.view(np.uint64) != w_tr.view(np.uint64))
        msg.append(f"trace: first difference at (scan, evaluation, column) {tuple(d[0])}: {g_tr[tuple(d[0])]!r} != {w_tr[tuple(d[0])]!r}")
    return "; ".join(msg[:6])


def _check(m, F, box, clouds, starts, p, res=RES):
    """refine and its trace equal the restatement in every byte; the records without a trace too."""
    got, g_tr = m.refine(clouds, starts, p, trace=True)
    want, w_tr = R.refine(F, box, res, clouds, api.refine_starts(starts), p)
    assert got.tobytes() == want.tobytes() and g_tr.tobytes() == w_tr.tobytes(), _explain(got, want, g_tr, w_tr)
    assert m.refine(clouds, starts, p).tobytes() == got.tobytes()
    return got, g_tr


def _starts():
    return np.stack([grid_start(o, RES) for o in START_OFFSETS] + [R.start_of(QUERY_POSE)])


# ------------------------------------------------------------------ 1. bytes against the restatement
def test_query_scan_from_five_starts(room):
    m, F, box = room
    got, tr = _check(m, F, box, [world().query] * 5, _starts(), R.params())
    assert set(got["status"]) <= {_abi.DPG_REFINE_CONVERGED, _abi.DPG_REFINE_MAX_ITERS} and (got["n_used"] == len(world().query)).all()
    assert (got["cost"] <= got["cost_start"]).all() and (got["cov_ok"] == 1).all()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, KCHUNK + 1])
def test_refine_by_cloud_size(room, n):
    m, F, box = room
    start = grid_start(START_OFFSETS[1], RES)
    got, _ = _check(m, F, box, [_cloud_of_size(n)], [start], R.params())
    assert int(got[0]["n_used"]) == n and (int(got[0]["status"]) == _abi.DPG_REFINE_NO_POINTS) == (n == 0)


def test_odd_inputs(room):
    """A cloud with non-finite and far points, a start off the map, max_iters 0 and 64 (tolerances 0, so
    that every step is taken)."""
    m, F, box = room
    w = world()
    bad = w.query[:200].copy()
    bad[3] = [np.nan, 1.0]
    bad[7] = [np.inf, -np.inf]
    bad[11] = [3e38, 0.5]
    bad[12] = [0.1 * 2 ** 29, 0.0]
    starts = _starts()
    got, _ = _check(m, F, box, [bad, w.query, np.full((5, 2), np.nan, f32)], [starts[0], R.start_of((900.0, -700.0, 0.3)), starts[0]], R.params())
    assert int(got[0]["n_used"]) == 197                    # all but the three; the far point rotates to within 2^29 cells
    assert (int(got[1]["status"]), int(got[1]["n_evals"]), int(got[1]["best_eval"])) == (_abi.DPG_REFINE_DEGENERATE, 1, 0)
    assert got[1]["pose"][0] == f32(900.0) and got[1]["pose"][1] == f32(-700.0) and int(got[2]["status"]) == _abi.DPG_REFINE_NO_POINTS
    got, tr = _check(m, F, box, [w.query] * 2, starts[:2], R.params(max_iters=0))
    assert (got["status"] == _abi.DPG_REFINE_MAX_ITERS).all() and (got["n_evals"] == 1).all() and tr.shape == (2, 1, 16)
    got, tr = _check(m, F, box, [w.query] * 2, starts[:2], R.params(max_iters=64, tol_cells=0.0, tol_angle=0.0))
    assert (got["status"] == _abi.DPG_REFINE_MAX_ITERS).all() and (got["n_evals"] == 65).all() and tr[:, 64, 4:].any()


def test_other_maps(ctx):
    """A corridor given as bytes (the best-iterate rule at work), a constant field and an empty map."""
    w = world()
    box = (0, 0, 80, 40)
    Fc = _corridor()
    cloud = _corridor_cloud(np.random.default_rng(5))
    m = api.FrozenMap.from_field(ctx, Fc, box, RES)
    got, _ = _check(m, Fc, box, [cloud, cloud], [R.start_of((4.03, 2.12, 0.015)), R.start_of((3.9, 1.95, -0.01))], R.params())
    assert int(got[0]["best_eval"]) < int(got[0]["n_evals"]) - 1
    m.close()
    flat = np.full((40, 80), 255, np.uint8)
    m = api.FrozenMap.from_field(ctx, flat, box, RES)
    got, _ = _check(m, flat, box, [cloud], [R.start_of((4.0, 2.0, 0.0))], R.params())
    assert (int(got[0]["status"]), int(got[0]["best_eval"]), float(got[0]["cost"])) == (_abi.DPG_REFINE_DEGENERATE, 0, 0.0)
    m.close()
    m = api.FrozenMap.from_field(ctx, np.zeros((0, 0), np.uint8), (4, 5, 0, 0), RES)
    got, _ = _check(m, np.zeros(0, np.uint8), (4, 5, 0, 0), [w.query, w.query[:0]], [R.start_of(GUESS), R.start_of(GUESS)], R.params())
    assert [int(s) for s in got["status"]] == [_abi.DPG_REFINE_DEGENERATE, _abi.DPG_REFINE_NO_POINTS]
    assert float(got[0]["cost"]) == 255.0 * 255.0 * len(w.query)
    # track_refine on the empty map: the tracker's all-zero winner, refined all the same
    tp = T.track_params(3, 2, 1)
    t, f = m.track_refine([w.query], [GUESS], tp, R.params())
    assert t.tobytes() == m.track([w.query], [GUESS], tp).tobytes() and int(t[0]["status"]) == _abi.DPG_LOC_NO_OVERLAP
    assert f.tobytes() == m.refine([w.query], t, R.params()).tobytes() and int(f[0]["status"]) == _abi.DPG_REFINE_DEGENERATE
    m.close()


# ------------------------------------------------------------------ 2. repeatability, batches and single calls
def test_batches_equal_single_calls(room):
    m, F, box = room
    w = world()
    clouds = [w.query, w.query[:77], w.query[:0], _cloud_of_size(KCHUNK + 5), w.query]
    starts = _starts()
    p = R.params()
    got, tr = m.refine(clouds, starts, p, trace=True)
    again, tr2 = m.refine(clouds, starts, p, trace=True)
    assert got.tobytes() == again.tobytes() and tr.tobytes() == tr2.tobytes()
    singles = [m.refine([c], s[None, :], p, trace=True) for c, s in zip(clouds, starts)]
    assert got.tobytes() == np.concatenate([r for r, _ in singles]).tobytes()
    assert tr.tobytes() == np.concatenate([t for _, t in singles]).tobytes()
    # cloud + offsets, with a leading part of the array that belongs to no scan
    pts = np.ascontiguousarray(np.concatenate([w.query[:13]] + clouds), f32)
    offs = 13 + np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    assert m.refine(pts, starts, p, offsets=offs).tobytes() == got.tobytes()
    assert len(m.refine([], np.zeros((0, 5), f32), p)) == 0


# ------------------------------------------------------------------ 3. track and refine in one enqueue
def test_track_refine(room):
    m, F, box = room
    w = world()
    tp, p = T.track_params(6, 5, 3, math.radians(1)), R.params()
    off = (900.0, -700.0, 0.3)                                                # wholly off the map: NO_OVERLAP, still refined
    clouds = [w.query, w.query[:77], w.query[:0], w.query, _cloud_of_size(KCHUNK + 5), w.query]
    guesses = [GUESS, (QUERY_POSE[0] - 0.4, QUERY_POSE[1] + 0.3, QUERY_POSE[2] - 0.02), GUESS,
               (QUERY_POSE[0] - 0.1, QUERY_POSE[1] - 0.5, QUERY_POSE[2] + 0.02), GUESS, off]
    for sel in ([0], list(range(6))):
        cl, gs = [clouds[i] for i in sel], [guesses[i] for i in sel]
        t, f = m.track_refine(cl, gs, tp, p)
        want_t = m.track(cl, gs, tp)
        assert t.tobytes() == want_t.tobytes() == T.track(F, box, RES, cl, gs, tp).tobytes()
        want_f = m.refine(cl, t, p)
        assert f.tobytes() == want_f.tobytes(), _explain(f, want_f)
        ref, _ = R.refine(F, box, RES, cl, R.starts_of(t), p)
        assert f.tobytes() == ref.tobytes(), _explain(f, ref)
        t2, f2 = m.track_refine(cl, gs, tp, p)
        assert t2.tobytes() == t.tobytes() and f2.tobytes() == f.tobytes()
    assert int(t[5]["status"]) == _abi.DPG_LOC_NO_OVERLAP and int(f[5]["status"]) == _abi.DPG_REFINE_DEGENERATE
    assert m.track(clouds, guesses, tp).tobytes() == t.tobytes()              # the tracker after a fused call: unchanged
    t0, f0 = m.track_refine([], np.zeros((0, 3), f32), tp, p)
    assert len(t0) == 0 and len(f0) == 0
    # the default window from GUESS: the refined pose is the accurate one
    t, f = m.track_refine([w.query], [GUESS])
    check_accuracy(f[0], R.starts_of(t)[0], RES)
    assert m.refine_kernel_ms() > 0.0 and m.track_kernel_ms() > 0.0


# ------------------------------------------------------------------ 4. the accuracy condition on the GPU's records
def test_accuracy_on_the_real_field(room):
    m, F, box = room
    starts = np.stack([grid_start(o, RES) for o in START_OFFSETS])
    got = m.refine([world().query] * len(starts), starts)
    for rec, start in zip(got, starts):
        check_accuracy(rec, start, RES)


# ------------------------------------------------------------------ 5. errors: nothing launched, nothing written
PATTERN = 0x5A5A5A5A


def _raw(m, fn, pts, offs, B, starts, p, n_out=None, trace_cap=None, handle="map", null=()):
    """The return code of dpg_fmap_refine / _trace on pre-filled outputs, and whether they are untouched."""
    out = np.full(max(B if n_out is None else n_out, 1) * 50, PATTERN, np.int32)
    tr = np.full(4096, 1.5, f64)
    pts, offs, st = np.ascontiguousarray(pts, f32), np.ascontiguousarray(offs, np.int64), np.ascontiguousarray(starts, f32)
    args = dict(m=m.handle if handle == "map" else None, pts=ptr(pts, C.c_float), offs=ptr(offs, C.c_int64), st=ptr(st, C.c_float),
                p=C.byref(p) if p is not None else None, out=_abi.vptr(out))
    for k in null:
        args[k] = None
    if fn == "trace":
        rc = lib().dpg_fmap_refine_trace(args["m"], args["pts"], args["offs"], B, args["st"], args["p"], args["out"], ptr(tr, C.c_double),
                                         len(tr) if trace_cap is None else trace_cap)
    else:
        rc = lib().dpg_fmap_refine(args["m"], args["pts"], args["offs"], B, args["st"], args["p"], args["out"])
    return rc, bool((out == PATTERN).all() and (tr == 1.5).all())


def _raw_track_refine(m, pts, offs, B, guesses, tp, rp):
    t_out, r_out = np.full(max(B, 1) * 12, PATTERN, np.int32), np.full(max(B, 1) * 50, PATTERN, np.int32)
    pts, offs, g = np.ascontiguousarray(pts, f32), np.ascontiguousarray(offs, np.int64), np.ascontiguousarray(guesses, f32)
    rc = lib().dpg_fmap_track_refine(m.handle, ptr(pts, C.c_float), ptr(offs, C.c_int64), B, ptr(g, C.c_float),
                                     C.byref(tp) if tp is not None else None, C.byref(rp) if rp is not None else None,
                                     _abi.vptr(t_out), _abi.vptr(r_out))
    return rc, bool((t_out == PATTERN).all() and (r_out == PATTERN).all())


def test_errors_write_nothing(room, ctx):
    m, F, box = room
    q = world().query
    n, p = len(q), R.params()
    st = _starts()[:1]
    ARG, SIZE = -1, -4
    for fn in ("refine", "trace"):
        for null in (("m",), ("offs",), ("st",), ("p",), ("out",), ("pts",)):
            assert _raw(m, fn, q, [0, n], 1, st, p, null=null) == (ARG, True), (fn, null)
        assert _raw(m, fn, q, [0, n], -1, st, p) == (ARG, True)
        assert _raw(m, fn, q, np.zeros(65537 + 1, np.int64), 65536, np.zeros((65536, 5), f32), p, n_out=1) == (SIZE, True)
        assert _raw(m, fn, q, [0, n, n - 1], 2, np.tile(st, (2, 1)), p) == (ARG, True)           # not monotone
        assert _raw(m, fn, q, [-1, n], 1, st, p) == (ARG, True)
        assert _raw(m, fn, q, [0, (1 << 23) + 1], 1, st, p) == (SIZE, True)
        assert _raw(m, fn, q, np.arange(10, dtype=np.int64) << 23, 9, np.tile(st, (9, 1)), p) == (SIZE, True)
        for bad in ([np.nan, 0, 0, 1, 0], [0, np.inf, 0, 1, 0], [0, 0, 0, np.nan, 0], [0, 0, 0, 1, np.inf], [0.1 * 2 ** 29, 0, 0, 1, 0],
                    [0, -1e9, 0, 1, 0], [0, 0, 0, 0.5, 0.4], [0, 0, 0, 1.2, 0.9], [0, 0, 0, 0, 0]):
            assert _raw(m, fn, q, [0, 10, n], 2, np.array([st[0], bad], f32), p) == (ARG, True), bad
        assert _raw(m, fn, q, [0, n], 1, [[0, 0, np.nan, 0.6, 0.8]], p)[0] == 0                  # theta is not read
        for bad in (R.params(max_iters=-1), R.params(max_iters=65), R.params(**{"lambda": -1.0}), R.params(**{"lambda": float("nan")}),
                    R.params(max_step_cells=0.0), R.params(max_step_angle=float("inf")), R.params(tol_cells=-1.0), R.params(tol_angle=float("nan"))):
            assert _raw(m, fn, q, [0, n], 1, st, bad) == (ARG, True)
    assert _raw(m, "trace", q, [0, n], 1, st, p, trace_cap=21 * 16 - 1) == (SIZE, True)
    assert _raw(m, "trace", q, [0, n], 1, st, p, trace_cap=21 * 16) == (0, False)
    assert _raw(m, "refine", q, [0], 0, st, p, n_out=1) == (0, True)                              # B = 0
    # track_refine: the tracker's errors and the refinement's
    tp, g = T.track_params(3, 2, 1), np.array([GUESS], f32)
    for bad_tp, bad_rp in ((T.track_params(65, 2, 1), p), (tp, R.params(max_iters=65)), (None, p), (tp, None)):
        assert _raw_track_refine(m, q, [0, n], 1, g, bad_tp, bad_rp) == (ARG, True)
    assert _raw_track_refine(m, q, [0, n, n - 1], 2, np.tile(g, (2, 1)), tp, p) == (ARG, True)
    assert _raw_track_refine(m, q, [0, n], 1, [[0.0, np.nan, 0.0]], tp, p) == (ARG, True)
    assert _raw_track_refine(m, q, [0, n], 1, [[0.1 * (2 ** 29 - 2), 0.0, 0.0]], tp, p) == (ARG, True)   # beyond 2^29 cells
    assert _raw_track_refine(m, q, np.zeros(65537 + 1, np.int64), 65536, np.zeros((65536, 3), f32), tp, p) == (SIZE, True)
    assert _raw_track_refine(m, q, [0, n], 1, g, tp, p) == (0, False)
    # DPG_ERR_STATE: the calls refuse a map of a multi-device context as dpg_fmap_track does (one shared check), but no
    # creator makes a map there, so no handle exists to pass; what can be asserted is that none can be made
    with api.Context(0, virtual=2) as multi:
        with pytest.raises(_abi.DpgError, match="single-device"):
            api.FrozenMap.from_field(multi, F, box, RES)


# ------------------------------------------------------------------ 6. through DpgSLAM on a loaded map
def test_dpgslam_field_refine_on_a_loaded_map(room, tmp_path):
    m, F, box = room
    w = world()
    path = tmp_path / "room.fmap"
    m.save(path)
    rng = np.random.default_rng(99)
    cp = _abi.default_change_params()
    cp.laser[0] = cp.laser[1] = cp.laser[2] = 0.0
    poses = [QUERY_POSE, (QUERY_POSE[0] + 0.3, QUERY_POSE[1] + 0.1, QUERY_POSE[2] + 0.05), (QUERY_POSE[0] + 0.6, QUERY_POSE[1] + 0.25, QUERY_POSE[2] + 0.1)]
    with api.Context(0) as c:
        slam = DpgSLAM(ctx=c, change_params=cp)                                # no node, no store: only the file
        fm = api.FrozenMap.load(c, path)
        slam.StartLocalization(fmap=fm, pose=GUESS, field_refine=True, icp_refine=False)
        assert slam.GetTrackedPoseCovariance() is None
        for k, pose in enumerate(poses):
            cloud = _cloud_at(pose, w.segs, rng)
            ranges = np.hypot(cloud[:, 0].astype(f64), cloud[:, 1].astype(f64)).astype(f32)
            if k:                                                              # the true motion as odometry
                slam.ObserveOdometry(f32(pose[:2]), f32(pose[2]))
            else:
                slam.ObserveOdometry(f32(poses[0][:2]), f32(poses[0][2]))
            slam.ObserveLaser(ranges, 0.0, RMAX, AMIN, AMAX)
            t, f = slam.last_track, slam.last_refine
            assert int(t["status"]) == _abi.DPG_LOC_OK and int(f["status"]) in (_abi.DPG_REFINE_CONVERGED, _abi.DPG_REFINE_MAX_ITERS)
            loc, ang = slam.GetPose()
            assert np.array_equal(loc, f["pose"][:2]) and ang == f["pose"][2] and len(slam.poses) == 0
            e_m, e_a = R.pose_error(f, pose)
            t_m, _ = R.pose_error(t, pose)
            print(f"scan {k}: track off {t_m:.4f} m, refined off {e_m:.4f} m {math.degrees(e_a):.3f} deg, {int(f['n_evals'])} evaluations")
            cov = slam.GetTrackedPoseCovariance()
            assert cov.shape == (3, 3) and np.array_equal(cov, cov.T) and (np.diag(cov) > 0).all()
            assert np.array_equal(cov[np.triu_indices(3)], f["cov"])
        slam.StopLocalization()
        fm.close()
