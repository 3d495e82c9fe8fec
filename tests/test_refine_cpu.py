"""The field refinement (dpg_fmap_refine) without a GPU: the ABI structs and the host helpers, the numpy
restatement tests/refine_ref.py against an independent scalar evaluation in plain Python floats, the
restatement's own properties, its accuracy in test_track.py's room, and DpgSLAM's field_refine over
fakes."""
import ctypes as C
import math

import numpy as np
import pytest

import csm_ref
import loc_ref as L
import refine_ref as R
from occ_grid_ref import c_round
from test_track_cpu import SCAN, FakeBackend, FakeStore, _cloud_of, _map_two_nodes, _rec, _room_field, _state
from dpgslam import _abi, api
from dpgslam._abi import lib, ptr
from dpgslam.slam import DpgSLAM

f32, f64 = np.float32, np.float64
BOX, RES = (-5, -7, 70, 60), 0.1


# ------------------------------------------------------------------ 1. ABI
def test_struct_sizes_and_defaults():
    assert C.sizeof(_abi.RefineParams) == 48 and C.sizeof(_abi.RefineResult) == 200 == _abi.REFINE_RESULT_DTYPE.itemsize
    assert [(n, getattr(_abi.RefineParams, n).offset) for n, _ in _abi.RefineParams._fields_] == \
        [("max_iters", 0), ("pad", 4), ("lambda_", 8), ("max_step_cells", 16), ("max_step_angle", 24), ("tol_cells", 32), ("tol_angle", 40)]
    offs = {n: getattr(_abi.RefineResult, n).offset for n, _ in _abi.RefineResult._fields_}
    assert offs == dict(pose=0, rot=12, status=20, n_evals=24, best_eval=28, n_used=32, pad=36, tu=40, tv=48, c=56, s=64, cost=72,
                        cost_start=80, sum_r=88, hess=96, cov=144, cov_ok=192, pad2=196)
    assert {n: _abi.REFINE_RESULT_DTYPE.fields[n][1] for n in _abi.REFINE_RESULT_DTYPE.names} == offs
    p = _abi.default_refine_params()
    assert (p.max_iters, p.pad, p.lambda_, p.max_step_cells, p.max_step_angle, p.tol_cells, p.tol_angle) == (20, 0, 1e-3, 1.0, 0.02, 1e-3, 1e-5)
    assert lib().dpg_refine_params_check(C.byref(p)) == 0 and lib().dpg_refine_params_check(None) == -1
    assert (_abi.DPG_REFINE_CONVERGED, _abi.DPG_REFINE_MAX_ITERS, _abi.DPG_REFINE_DEGENERATE, _abi.DPG_REFINE_NO_POINTS) == (0, 1, 2, 3)


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("field,good,bad", [
    ("max_iters", (0, 1, 64), (-1, 65)),
    ("lambda_", (0.0, 1e-3, 1e6), (-1e-9, NAN, INF, -INF)),
    ("max_step_cells", (1e-9, 1.0, 50.0), (0.0, -1.0, NAN, INF)),
    ("max_step_angle", (1e-9, 0.02, 3.0), (0.0, -0.1, NAN, INF)),
    ("tol_cells", (0.0, 1e-3, 2.0), (-1e-9, NAN, INF)),
    ("tol_angle", (0.0, 1e-5, 1.0), (-1e-9, NAN, INF)),
])
def test_refine_params_check(field, good, bad):
    for v in good:
        p = _abi.default_refine_params()
        setattr(p, field, v)
        assert lib().dpg_refine_params_check(C.byref(p)) == 0, (field, v)
    for v in bad:
        p = _abi.default_refine_params()
        setattr(p, field, v)
        assert lib().dpg_refine_params_check(C.byref(p)) == -1, (field, v)


# ------------------------------------------------------------------ 2. the host helpers
def test_refine_start_and_angle():
    lp = _abi.default_loc_params()
    lp.half_a = 0
    for th in (0.0, 1.106, -2.5, 3.1415927, 100.0, -0.0):
        pose = np.array([1.25, -3.5, th], f32)
        out = np.zeros(5, f32)
        assert lib().dpg_refine_start(ptr(pose, C.c_float), ptr(out, C.c_float)) == 0
        assert out[:3].tobytes() == pose.tobytes()
        if th != 0.0 or math.copysign(1.0, th) > 0:        # dpg_loc_rotations' rule (which adds 0 steps: -0.0 becomes +0.0 there)
            assert out[3:].tobytes() == api.loc_rotations(pose[2], lp)[0].tobytes()
        assert out[3] == f32(math.cos(float(pose[2]))) and out[4] == f32(math.sin(float(pose[2])))
        assert out.tobytes() == R.start_of(pose).tobytes() == api.refine_starts(pose[None, :])[0].tobytes()
    assert lib().dpg_refine_start(None, ptr(np.zeros(5, f32), C.c_float)) == -1
    for c, s in ((1.0, 0.0), (0.3, -0.8), (-1.0, 1e-17), (0.0, 0.0), (-2.0, -3.0)):
        assert lib().dpg_refine_angle(c, s) == f32(math.atan2(s, c))
    rec = np.zeros(2, _abi.TRACK_RESULT_DTYPE)
    rec["pose"], rec["rot"] = [[1, 2, 3], [4, 5, 6]], [[0.6, 0.8], [1.0, 0.0]]
    assert api.refine_starts(rec).tobytes() == f32([[1, 2, 3, 0.6, 0.8], [4, 5, 6, 1.0, 0.0]]).tobytes() == R.starts_of(rec).tobytes()


# ------------------------------------------------------------------ 3. the restatement against a scalar evaluation
def _F_at(F, box, ix, iy):
    return float(F[iy][ix]) if 0 <= ix < box[2] and 0 <= iy < box[3] else 0.0


def _scalar_eval(F, box, ires, cloud, state):
    """Plain Python floats, point by point, in the contract's order: lanes, fold, (W0 + W1) + (W2 + W3)."""
    tu, tv, c, s = (float(v) for v in state)
    lanes = [[0.0] * 11 for _ in range(256)]
    n_used = 0
    for i, (x, y) in enumerate(cloud):
        if not (math.isfinite(x) and math.isfinite(y)):
            continue
        px, py = float(x) * ires, float(y) * ires
        rx, ry = (c * px) - (s * py), (s * px) + (c * py)
        u, v = rx + tu, ry + tv
        if not (abs(u) < 2.0 ** 29 and abs(v) < 2.0 ** 29):
            continue
        iu, iv = math.floor(u), math.floor(v)
        fu, fv = u - iu, v - iv
        au, av = 1.0 - fu, 1.0 - fv
        F00, F10, F01, F11 = _F_at(F, box, iu, iv), _F_at(F, box, iu + 1, iv), _F_at(F, box, iu, iv + 1), _F_at(F, box, iu + 1, iv + 1)
        M = (av * ((au * F00) + (fu * F10))) + (fv * ((au * F01) + (fu * F11)))
        gu = (av * (F10 - F00)) + (fv * (F11 - F01))
        gv = (au * (F01 - F00)) + (fu * (F11 - F10))
        r = 255.0 - M
        jt = (gv * rx) - (gu * ry)
        t = lanes[i % 256]
        for j, q in enumerate((gu * gu, gu * gv, gu * jt, gv * gv, gv * jt, jt * jt, gu * r, gv * r, jt * r, r * r, r)):
            t[j] += q
        n_used += 1
    W = []
    for g in range(4):
        p = [list(t) for t in lanes[64 * g:64 * g + 64]]
        for st in (32, 16, 8, 4, 2, 1):
            for l in range(st):
                for j in range(11):
                    p[l][j] += p[l + st][j]
        W.append(p[0])
    return [(W[0][j] + W[1][j]) + (W[2][j] + W[3][j]) for j in range(11)], n_used


def _scalar_solve(H, lam, b):
    eps = 1e-12
    H00, H01, H02, H11, H12, H22 = H
    D1, D2, d0 = H11 + (lam * H11), H22 + (lam * H22), H00 + (lam * H00)
    if not d0 > 0:
        return None
    l10, l20 = H01 / d0, H02 / d0
    d1 = D1 - (l10 * H01)
    if not d1 > eps * D1:
        return None
    e12 = H12 - (l20 * H01)
    l21 = e12 / d1
    d2 = (D2 - (l20 * H02)) - (l21 * e12)
    if not d2 > eps * D2:
        return None
    y0 = b[0]
    y1 = b[1] - (l10 * y0)
    y2 = (b[2] - (l20 * y0)) - (l21 * y1)
    z2 = y2 / d2
    z1 = (y1 / d1) - (l21 * z2)
    z0 = ((y0 / d0) - (l10 * z1)) - (l20 * z2)
    return z0, z1, z2


def _scalar_refine(F, box, res, cloud, start, p):
    """The loop and the record in plain floats."""
    ires = 1.0 / res
    st = [float(v) for v in np.asarray(start, f32)]
    state = ((st[0] * ires) - float(box[0]), (st[1] * ires) - float(box[1]), st[3], st[4])
    cloud = [(float(x), float(y)) for x, y in np.asarray(cloud, f32).reshape(-1, 2)]
    K, best, S0, status = int(p.max_iters), None, None, None
    clamp = lambda z, m: m if z > m else (-m if z < -m else z)      # noqa: E731
    for k in range(K + 1):
        S, n_used = _scalar_eval(F, box, ires, cloud, state)
        if k == 0:
            S0 = list(S)
        if k == 0 or S[9] < best[2][9]:
            best = (k, state, S, n_used)
        if k == 0 and n_used == 0:
            status = 3
        elif k == K:
            status = 1
        else:
            z = _scalar_solve(S[:6], p.lambda_, S[6:9])
            if z is None or not all(math.isfinite(v) for v in z):
                status = 2
            else:
                du, dv, dt = clamp(z[0], p.max_step_cells), clamp(z[1], p.max_step_cells), clamp(z[2], p.max_step_angle)
                if abs(du) < p.tol_cells and abs(dv) < p.tol_cells and abs(dt) < p.tol_angle:
                    status = 0
                else:
                    tu, tv, c, s = state
                    a = dt * 0.5
                    q = a * a
                    den = 1.0 + q
                    cd, sd = (1.0 - q) / den, (a + a) / den
                    state = (tu + du, tv + dv, (c * cd) - (s * sd), (s * cd) + (c * sd))
        if status is not None:
            break
    n_evals = k + 1
    k, state, S, n_used = best
    r = np.zeros((), _abi.REFINE_RESULT_DTYPE)
    r["pose"] = [f32((state[0] + float(box[0])) * res), f32((state[1] + float(box[1])) * res), f32(math.atan2(state[3], state[2]))]
    r["rot"] = [f32(state[2]), f32(state[3])]
    r["status"], r["n_evals"], r["best_eval"], r["n_used"] = status, n_evals, k, n_used
    r["tu"], r["tv"], r["c"], r["s"] = state
    r["cost"], r["cost_start"], r["sum_r"], r["hess"] = S[9], S0[9], S[10], S[:6]
    s2 = S[9] / float(max(n_used - 3, 1))
    cols = [_scalar_solve(S[:6], 0.0, e) for e in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))]
    if all(z is not None for z in cols):
        rr = res * res
        cov = [(s2 * cols[0][0]) * rr, (s2 * cols[1][0]) * rr, (s2 * cols[2][0]) * res, (s2 * cols[1][1]) * rr, (s2 * cols[2][1]) * res,
               s2 * cols[2][2]]
        if all(math.isfinite(v) for v in cov):
            r["cov"], r["cov_ok"] = cov, 1
    return r, S0


TRUE_POSE = (3.0, 2.3, 0.4)


def _wall_cloud(n):
    """n points of the room field's walls seen from TRUE_POSE, with a little noise."""
    base = _cloud_of(_room_field(), BOX, RES, TRUE_POSE)
    rng = np.random.default_rng(n)
    idx = rng.permutation(len(base))
    c = np.concatenate([base[idx]] * (n // len(base) + 1))[:n] + rng.normal(0, 0.01, (n, 2)).astype(f32)
    return np.ascontiguousarray(c, f32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 600, "nan"])
def test_restatement_equals_the_scalar_evaluation(n):
    F = _room_field()
    if n == "nan":
        cloud = _wall_cloud(300)
        cloud[5] = [np.nan, 0.0]
        cloud[77] = [1.0, np.inf]
        cloud[78] = [3e38, 1.0]            # finite, but |u| is beyond 2^29
    else:
        cloud = _wall_cloud(n)
    start = R.start_of((TRUE_POSE[0] + 0.06, TRUE_POSE[1] - 0.05, TRUE_POSE[2] + 0.01))
    p = R.params(max_iters=4)
    ires, state = R.start_state(BOX, RES, start)
    used, T = R.terms(F, BOX, ires, cloud, state)
    S, n_used = R.sums(used, T)
    S_want, n_want = _scalar_eval(F.tolist(), BOX, 1.0 / RES, [(float(x), float(y)) for x, y in cloud], state)
    assert n_used == n_want and (n_used == len(cloud) if n != "nan" else n_used == len(cloud) - 3)
    assert np.array(S, f64).tobytes() == np.array(S_want, f64).tobytes()
    rec, trace = R.refine_one(F, BOX, RES, cloud, start, p)
    want, S0 = _scalar_refine(F.tolist(), BOX, RES, cloud, start, p)
    assert trace[0, 4:15].tobytes() == np.array(S0, f64).tobytes()
    assert rec.tobytes() == want.tobytes(), (rec, want)
    assert 1 <= int(rec["n_evals"]) <= 5 and not trace[int(rec["n_evals"]):].any() and trace[int(rec["n_evals"]) - 1, 4:].any()


# ------------------------------------------------------------------ 4. properties of the restatement
def _corridor(w=80, h=40):
    """Two parallel walls along x with a smooth profile across and a few bytes of texture along: only
    that texture speaks about x (a profile constant in x has gu = 0 exactly and is DEGENERATE at once)."""
    F = np.zeros((h, w), np.uint8)
    prof, xs = [255, 200, 120, 50], np.arange(w)
    for y0 in (10, 30):
        for d, v in enumerate(prof):
            for yy in (y0 - d, y0 + d):
                F[yy] = np.maximum(F[yy], (v - ((xs * 7 + yy * 3) % 5) * 3).astype(np.uint8))
    return F


def _corridor_cloud(rng, n=240):
    """Points on the two walls (map cells y = 10 and y = 30, box origin 0) seen from (4.0, 2.0, 0.0)."""
    xs = rng.uniform(0.5, 7.5, n)
    ys = np.where(np.arange(n) % 2 == 0, 1.0, 3.0) + rng.normal(0, 0.01, n)
    return np.stack([xs - 4.0, ys - 2.0], 1).astype(f32)


def test_properties_of_the_restatement():
    F = _room_field()
    cloud = _wall_cloud(300)
    p = R.params()
    for off in ((0.06, -0.05, 0.01), (0.0, 0.0, 0.0), (-0.12, 0.08, -0.02), (0.4, 0.4, 0.1)):
        rec, tr = R.refine_one(F, BOX, RES, cloud, R.start_of(np.add(TRUE_POSE, off)), p)
        assert float(rec["cost"]) <= float(rec["cost_start"]) and float(rec["cost_start"]) == tr[0, 13]
        assert float(rec["cost"]) == tr[int(rec["best_eval"]), 13] == tr[:int(rec["n_evals"]), 13].min()
    # nothing to descend on: DEGENERATE at evaluation 0, the start back
    start = R.start_of(TRUE_POSE)
    for Fx, box, st in ((np.full((60, 70), 255, np.uint8), BOX, start), (F, BOX, R.start_of((500.0, -300.0, 0.4))),
                        (np.zeros(0, np.uint8), (4, 5, 0, 0), start)):
        rec, tr = R.refine_one(Fx, box, RES, cloud, st, p)
        assert (int(rec["status"]), int(rec["n_evals"]), int(rec["best_eval"])) == (_abi.DPG_REFINE_DEGENERATE, 1, 0)
        assert np.array_equal(rec["rot"], st[3:]) and not int(rec["cov_ok"]) and not rec["cov"].any()
        assert abs(float(rec["pose"][0]) - float(st[0])) < 1e-5 * max(1.0, abs(float(st[0]))) and int(rec["n_used"]) == len(cloud)
    # only non-finite points
    bad = np.full((7, 2), np.nan, f32)
    bad[3] = [np.inf, 1.0]
    rec, _ = R.refine_one(F, BOX, RES, bad, start, p)
    assert (int(rec["status"]), int(rec["n_evals"]), int(rec["n_used"])) == (_abi.DPG_REFINE_NO_POINTS, 1, 0)
    rec, _ = R.refine_one(F, BOX, RES, cloud[:0], start, p)
    assert int(rec["status"]) == _abi.DPG_REFINE_NO_POINTS
    # max_iters = 0: one evaluation
    rec, tr = R.refine_one(F, BOX, RES, cloud, start, R.params(max_iters=0))
    assert (int(rec["status"]), int(rec["n_evals"]), int(rec["best_eval"])) == (_abi.DPG_REFINE_MAX_ITERS, 1, 0) and tr.shape == (1, 16)
    # a good start in the room: it converges, and the covariance is that of a pinned-down pose
    rec, _ = R.refine_one(F, BOX, RES, cloud, R.start_of(np.add(TRUE_POSE, (0.06, -0.05, 0.01))), p)
    assert int(rec["status"]) == _abi.DPG_REFINE_CONVERGED and int(rec["cov_ok"]) == 1
    assert rec["cov"][0] > 0 and rec["cov"][3] > 0 and rec["cov"][5] > 0


def test_corridor_exercises_the_best_iterate_rule():
    """Between two walls the cost does not fall monotonically: x is free, the damped step slides along
    the corridor, and the last iterate is not the best one."""
    F, box = _corridor(), (0, 0, 80, 40)
    cloud = _corridor_cloud(np.random.default_rng(5))
    rec, tr = R.refine_one(F, box, RES, cloud, R.start_of((4.03, 2.12, 0.015)), R.params())
    n, best = int(rec["n_evals"]), int(rec["best_eval"])
    print(f"corridor: status {int(rec['status'])}, best_eval {best} of {n}, costs {tr[:n, 13]}")
    assert best < n - 1, "the case must end on an iterate that is not its best"
    assert float(rec["cost"]) == tr[:n, 13].min() <= float(rec["cost_start"])
    assert abs(float(rec["pose"][1]) - 2.0) < RES / 4 and abs(float(rec["pose"][2])) < math.radians(0.25)


# ------------------------------------------------------------------ 5. the accuracy condition in test_track.py's room
NB = 360
NODE_POSES = [(2.0, 2.0, 0.3), (5.5, 1.2, 1.9), (10.5, 2.0, -2.5), (10.0, 7.0, 0.8), (5.0, 7.5, -1.0), (1.5, 6.5, 2.6)]
QUERY_POSE = (6.43, 4.57, 1.106)
GUESS = (QUERY_POSE[0] + 0.33, QUERY_POSE[1] - 0.21, QUERY_POSE[2] + 0.04)
# GUESS and three more offsets inside the default track window (10 cells, 5 degrees) of QUERY_POSE
START_OFFSETS = [(0.33, -0.21, 0.04), (-0.25, 0.15, -0.03), (0.1, 0.3, 0.02), (-0.05, -0.35, -0.04)]
STEP = math.radians(0.5)


def room_world(res=0.1):
    """test_track.py's world on the CPU: the six node scans and the query scan in its generator's order,
    and the likelihood field (loc_ref.field) of the grid whose occupied cells are the keys of the
    nodes' end points -- the store's grid restated from the end points, as test_track.py's docstrings do."""
    rng = np.random.default_rng(4711)
    segs = csm_ref._segments()
    clouds = [csm_ref._scan(p, segs, NB, 0.01, rng) for p in NODE_POSES]
    query = np.ascontiguousarray(csm_ref._scan(QUERY_POSE, segs, NB, 0.01, rng), f32)
    world = []
    for (x, y, th), c in zip(NODE_POSES, clouds):
        c = c.astype(f64)
        world.append(np.stack([x + math.cos(th) * c[:, 0] - math.sin(th) * c[:, 1], y + math.sin(th) * c[:, 0] + math.cos(th) * c[:, 1]], 1))
    k = c_round(np.concatenate(world) / res).astype(np.int64)
    x0, y0 = k.min(0) - 1
    w, h = k.max(0) - (x0, y0) + 2
    occ = np.full((h, w), -1, np.int8)
    occ[k[:, 1] - y0, k[:, 0] - x0] = 100
    lp = _abi.default_loc_params()
    lp.resolution = res
    return L.field(occ, lp, res), (int(x0), int(y0), int(w), int(h)), query


def grid_start(off, res):
    """The start a track would hand over: the cell centre and the angle step nearest QUERY_POSE + off."""
    x, y, th = np.add(QUERY_POSE, off)
    return R.start_of((round(x / res) * res, round(y / res) * res, round(th / STEP) * STEP))


def check_accuracy(rec, start, res):
    """The condition of the issue: within res / 4 and 0.25 degrees of QUERY_POSE, and nearer than the start."""
    e_m, e_a = R.pose_error(rec, QUERY_POSE)
    s_m = math.hypot(float(start[0]) - QUERY_POSE[0], float(start[1]) - QUERY_POSE[1])
    s_a = abs(math.remainder(float(start[2]) - QUERY_POSE[2], 2 * math.pi))
    print(f"start off {s_m:.4f} m {math.degrees(s_a):.3f} deg -> refined off {e_m:.5f} m {math.degrees(e_a):.4f} deg, "
          f"status {int(rec['status'])}, {int(rec['n_evals'])} evaluations, best {int(rec['best_eval'])}")
    assert int(rec["status"]) in (_abi.DPG_REFINE_CONVERGED, _abi.DPG_REFINE_MAX_ITERS)
    assert e_m <= res / 4 and e_a <= math.radians(0.25), (e_m, e_a)
    assert e_m < s_m and e_a < s_a + 1e-12, (e_m, s_m, e_a, s_a)


@pytest.mark.parametrize("res", [0.1, 0.05])
def test_accuracy_of_the_restatement_in_the_room(res):
    F, box, query = room_world(res)
    for off in START_OFFSETS:
        start = grid_start(off, res)
        rec, _ = R.refine_one(F, box, res, query, start, R.params())
        check_accuracy(rec, start, res)


# ------------------------------------------------------------------ 6. DpgSLAM over fakes
class FakeRefineMap:
    def __init__(self, pairs):
        self.pairs, self.calls, self.closed = list(pairs), [], False

    def track(self, clouds, guesses, params=None):
        raise AssertionError("field_refine goes through track_refine")

    def track_refine(self, clouds, guesses, track_params=None, refine_params=None):
        self.calls.append((np.array(clouds[0]), np.array(guesses[0], f32), track_params, refine_params))
        t, f = self.pairs.pop(0)
        return np.array([t]), np.array([f])

    def close(self):
        self.closed = True


def _ref(pose=(0.0, 0.0, 0.0), status=_abi.DPG_REFINE_CONVERGED, cov=(4e-4, 1e-5, 2e-6, 3e-4, -1e-6, 5e-5), cov_ok=1):
    r = np.zeros((), _abi.REFINE_RESULT_DTYPE)
    r["pose"], r["status"], r["cov"], r["cov_ok"] = pose, status, cov, cov_ok
    return r


class NoIcpBackend(FakeBackend):
    ctx = None


def test_slam_field_refine_over_fakes():
    pairs = [(_rec((2.0, 0.5, 0.1)), _ref((2.03, 0.47, 0.104))),                                   # refined: accepted
             (_rec((3.0, 0.5, 0.1)), _ref((9.0, 9.0, 1.0), status=_abi.DPG_REFINE_DEGENERATE)),    # falls back to the track
             (_rec((7.0, 7.0, 1.0), score=100), _ref((7.01, 7.01, 1.0))),                          # a refused track
             (_rec((4.0, 0.0, 0.0)), _ref((4.02, 0.01, 0.003), status=_abi.DPG_REFINE_MAX_ITERS, cov_ok=0, cov=(0,) * 6))]
    fmap = FakeRefineMap(pairs)
    be = NoIcpBackend(FakeStore(fmap))
    slam = DpgSLAM(backend=be)
    _map_two_nodes(slam)
    before = _state(slam, be)
    tp, rp = _abi.default_track_params(), R.params(max_iters=7)
    assert slam.GetTrackedPoseCovariance() is None
    slam.StartLocalization(track_params=tp, min_response=0.3, field_refine=rp)      # icp_refine's default: no ICP is needed or run
    assert slam.last_refine is None and slam.GetTrackedPoseCovariance() is None
    slam.ObserveOdometry(np.array([2.0, 0.25], f32), f32(0.05))
    slam.ObserveLaser(SCAN, 0.0, 10.0, -math.pi, math.pi)
    assert fmap.calls[0][2] is tp and fmap.calls[0][3] is rp
    loc, ang = slam.GetPose()
    assert np.array_equal(loc, f32([2.03, 0.47])) and ang == f32(0.104)
    assert np.array_equal(slam.last_track["pose"], f32([2.0, 0.5, 0.1])) and np.array_equal(slam.last_refine["pose"], f32([2.03, 0.47, 0.104]))
    cov = slam.GetTrackedPoseCovariance()
    assert cov.shape == (3, 3) and np.array_equal(cov, cov.T)
    assert np.array_equal(cov[np.triu_indices(3)], [4e-4, 1e-5, 2e-6, 3e-4, -1e-6, 5e-5])
    # DEGENERATE: the track's pose, and no covariance
    slam.ObserveLaser(SCAN, 0.0, 10.0, -math.pi, math.pi)
    loc, ang = slam.GetPose()
    assert np.array_equal(loc, f32([3.0, 0.5])) and ang == f32(0.1) and slam.GetTrackedPoseCovariance() is None
    assert int(slam.last_refine["status"]) == _abi.DPG_REFINE_DEGENERATE
    # a refused track: the pose dead-reckons on from the last accepted one
    slam.ObserveOdometry(np.array([3.0, 0.25], f32), f32(0.05))
    slam.ObserveLaser(SCAN, 0.0, 10.0, -math.pi, math.pi)
    want = api.transform_point(api.inverse_transform_point(f32([3.0, 0.25, 0.05]), f32([2.0, 0.25, 0.05])), f32([3.0, 0.5, 0.1]))
    loc, ang = slam.GetPose()
    assert np.allclose([loc[0], loc[1], ang], want, atol=1e-5) and np.array_equal(slam.last_refine["pose"], f32([7.01, 7.01, 1.0]))
    # MAX_ITERS is accepted; cov_ok 0 gives no covariance
    slam.ObserveLaser(SCAN, 0.0, 10.0, -math.pi, math.pi)
    assert np.array_equal(slam.GetPose()[0], f32([4.02, 0.01])) and slam.GetTrackedPoseCovariance() is None
    slam.StopLocalization()
    assert fmap.closed and _state(slam, be) == before and len(fmap.calls) == 4 and slam.GetTrackedPoseCovariance() is None
    slam.ObserveLaser(SCAN, 0.0, 10.0, -math.pi, math.pi)
    assert len(slam.poses) == 3
    # True means the defaults; a map without track_refine is refused
    fm2 = FakeRefineMap([(_rec((1.0, 2.0, 0.3)), _ref((1.01, 2.02, 0.31)))])
    slam.StartLocalization(fmap=fm2, field_refine=True, icp_refine=False)
    slam.ObserveLaser(SCAN, 0.0, 10.0, -math.pi, math.pi)
    assert bytes(fm2.calls[0][3]) == bytes(_abi.default_refine_params()) and np.array_equal(slam.GetPose()[0], f32([1.01, 2.02]))
    slam.StopLocalization()
    assert not fm2.closed

    class TrackOnly:
        def track(self, *a):
            return None
    with pytest.raises(NotImplementedError, match=r"needs a `track_refine\(.*\)` method on the map; TrackOnly has none"):
        slam.StartLocalization(fmap=TrackOnly(), field_refine=True, icp_refine=False)
