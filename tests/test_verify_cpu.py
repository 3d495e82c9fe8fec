"""Loop-closure verification, host side (no GPU): the numpy reference (tests/verify_ref.py) pinned by
hand, the host functions of dpg_host.c (defaults, parameter check, sensor key, LDS bytes), the ABI
structs against the header compiled as C, the acceptance rule, DpgSLAM's backend protocol, and the
reference alone with the CPU oracle's ICP on the room: the converged alignment 1.4 m off is rejected,
the true one accepted."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import csm_ref
import verify_ref as V
from dpgslam import _abi, api
from dpgslam._abi import lib, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
ERR_ARG = -1   # DPG_ERR_ARG


def _params(**kw):
    p = _abi.default_verify_params()
    for k, v in kw.items():
        if k == "sensor":
            p.sensor[0], p.sensor[1] = v
        else:
            setattr(p, k, v)
    return p


def _unit(**kw):
    """One metre per cell, the sensor at the origin, no occupied spread: keys are the coordinates."""
    kw = dict(dict(resolution=1.0, sensor=(0.0, 0.0), occ_radius=0, half_cells=8), **kw)
    return _params(**kw)


def _cells(T, state):
    H = T.shape[0] // 2
    v, u = np.nonzero(T == state)
    return sorted(zip((u - H).tolist(), (v - H).tolist()))


# ------------------------------------------------------------------ the reference, by hand
def test_reference_one_ray_marks_the_cells_of_the_formula():
    """Model point at key (5, 2), sensor key (0, 0): n = 5, off_x = i, off_y = floor((4 i + 5) / 10) =
    0, 0, 1, 1, 2 for i = 0 .. 4; the end cell (5, 2) is not free (it is occupied)."""
    T = V.table(np.array([[5.0, 2.0]], np.float32), _unit())
    assert _cells(T, 1) == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2)]
    assert _cells(T, 2) == [(5, 2)]
    assert V.free_cells((0, 0), (5, 2)) == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2)]
    # the same ray in the other three quadrants and with the axes exchanged: signs and roles mirror
    assert _cells(V.table(np.array([[-5.0, 2.0]], np.float32), _unit()), 1) == sorted([(0, 0), (-1, 0), (-2, 1), (-3, 1), (-4, 2)])
    assert _cells(V.table(np.array([[5.0, -2.0]], np.float32), _unit()), 1) == sorted([(0, 0), (1, 0), (2, -1), (3, -1), (4, -2)])
    assert _cells(V.table(np.array([[-2.0, -5.0]], np.float32), _unit()), 1) == sorted([(0, 0), (0, -1), (-1, -2), (-1, -3), (-2, -4)])


def test_reference_diagonal_axis_tie_and_zero_length_rays():
    p = _unit()
    assert _cells(V.table(np.array([[4.0, -4.0]], np.float32), p), 1) == [(0, 0), (1, -1), (2, -2), (3, -3)]       # exact diagonal
    assert _cells(V.table(np.array([[3.0, 0.0]], np.float32), p), 1) == [(0, 0), (1, 0), (2, 0)]                   # axis rays, both signs
    assert _cells(V.table(np.array([[-3.0, 0.0]], np.float32), p), 1) == [(-2, 0), (-1, 0), (0, 0)]
    assert _cells(V.table(np.array([[0.0, 2.0]], np.float32), p), 1) == [(0, 0), (0, 1)]
    assert _cells(V.table(np.array([[0.0, -2.0]], np.float32), p), 1) == [(0, -1), (0, 0)]
    # a tie: d = (2, 1), i = 1: 2 i |dy| + n = 4 = 2 n, so i dy / n = 1 / 2 rounds up to 1, in magnitude for both signs
    assert V.free_cells((0, 0), (2, 1)) == [(0, 0), (1, 1)]
    assert V.free_cells((0, 0), (-2, -1)) == [(0, 0), (-1, -1)]
    assert _cells(V.table(np.array([[2.0, 1.0], [-2.0, -1.0]], np.float32), p), 1) == [(-1, -1), (0, 0), (1, 1)]
    assert int(V.ray_offsets(1, 2, 1)) == 1 and int(V.ray_offsets(-1, 2, 1)) == -1 and int(V.ray_offsets(1, 4, 1)) == 0
    # n = 0: the point in the sensor's own cell marks no free cell; its cell is occupied
    T = V.table(np.array([[0.2, -0.3]], np.float32), p)
    assert _cells(T, 1) == [] and _cells(T, 2) == [(0, 0)]
    # the sensor off the origin: the rays start at its key
    q = _unit(sensor=(2.0, -1.0))
    assert V.sensor_key(q) == (2, -1) == api.verify_sensor_key(q)
    assert _cells(V.table(np.array([[5.0, -1.0]], np.float32), q), 1) == [(2, -1), (3, -1), (4, -1)]
    # non-finite and huge points count for nothing
    T = V.table(np.array([[np.nan, 1.0], [1.0, np.inf], [6e8, 0.0], [0.0, 2.0]], np.float32), p)
    assert _cells(T, 1) == [(0, 0), (0, 1)] and _cells(T, 2) == [(0, 2)]


def test_reference_clipping_and_the_step_bound():
    """A point outside the table marks the clipped part of its ray only; a point with a key near 2^29
    gives the cells of the unbounded loop: off along the longer axis is i itself, so past i = 2H the
    ray has left the table for good."""
    p = _unit(half_cells=3)
    T = V.table(np.array([[10.0, 4.0]], np.float32), p)           # n = 10, off_y = floor((8 i + 10) / 20)
    assert _cells(T, 1) == [(0, 0), (1, 0), (2, 1), (3, 1)] and _cells(T, 2) == []
    q = _unit(half_cells=3, sensor=(-3.0, 3.0))                   # the sensor in a corner: the longest walk inside, 2H cells
    assert _cells(V.table(np.array([[40.0, 3.0]], np.float32), q), 1) == [(u, 3) for u in range(-3, 4)]
    far = np.array([[5.3e8, 2.1e8], [-5.0e8, 5.3e8], [1.0e8, -5.36e8]], np.float32)
    kx, ky, ok = csm_ref.keys(far, 1.0)
    assert ok.all() and np.abs(ky[2]) > 2 ** 29 - 2 ** 20
    for prm in (p, q):
        want = V.table(far, prm)
        assert want.any()
        np.testing.assert_array_equal(want, V.table(far, prm, max_steps=5000))   # far more steps: the same cells
        a = V.sensor_key(prm)
        rng = np.random.default_rng(2)
        for k in range(3):                                                       # and anywhere along the whole ray: outside
            d = np.array([kx[k] - a[0], ky[k] - a[1]])
            n = int(np.abs(d).max())
            i = np.concatenate([rng.integers(2 * 3 + 1, n, 2000), [2 * 3 + 1, n - 1]])
            u, v = a[0] + V.ray_offsets(d[0], n, i), a[1] + V.ray_offsets(d[1], n, i)
            assert (np.maximum(np.abs(u), np.abs(v)) > 3).all()
            major = 0 if abs(d[0]) >= abs(d[1]) else 1
            assert (np.abs(V.ray_offsets(d[major], n, i)) == i).all()


def test_reference_occupied_wins_and_radius_zero():
    p = _unit(occ_radius=1)
    T = V.table(np.array([[4.0, 0.0], [2.0, 0.0]], np.float32), p)
    # the ray to (4, 0) crosses (2, 0) and its neighbours (1, 0), (3, 0), which the nearer point occupies
    assert [int(T[8, 8 + u]) for u in range(0, 6)] == [1, 2, 2, 2, 2, 2]
    assert _cells(T, 2) == sorted({(2 + ox, oy) for ox in (-1, 0, 1) for oy in (-1, 0, 1) if ox * ox + oy * oy <= 1} |
                                  {(4 + ox, oy) for ox in (-1, 0, 1) for oy in (-1, 0, 1) if ox * ox + oy * oy <= 1})
    T0 = V.table(np.array([[4.0, 0.0], [2.0, 0.0]], np.float32), _unit(occ_radius=0))
    assert [int(T0[8, 8 + u]) for u in range(0, 6)] == [1, 1, 2, 1, 2, 0]
    # a point beyond the table still spreads into it
    T1 = V.table(np.array([[9.0, 0.0]], np.float32), _unit(occ_radius=2))
    assert _cells(T1, 2) == [(7, 0), (8, -1), (8, 0), (8, 1)]


def test_reference_a_cloud_supports_itself_under_the_identity():
    rm = csm_ref.room()
    p = _abi.default_verify_params()
    ident = np.array([1, 0, 0, 0, 1, 0], np.float32)
    for d in (0, 1):
        np.testing.assert_array_equal(V.moved(rm.clouds[0], ident, d), rm.clouds[0])
    r = V.result(rm.clouds[0], rm.clouds[0], ident, p)
    assert r["n_pts"].tolist() == [360, 360] and r["n_in"].tolist() == [360, 360]
    assert r["n_support"].tolist() == r["n_in"].tolist() and r["n_free"].tolist() == [0, 0]
    assert r["status"] == _abi.DPG_VERIFY_OK and not r["pad"].any()
    # direction 1 is the inverse of direction 0 for a rigid T, up to float rounding
    T = csm_ref.guess_of(0.7, -0.4, 0.3)
    back = V.moved(V.moved(rm.clouds[1], T, 0), T, 1)
    assert np.abs(back - rm.clouds[1]).max() < 1e-5
    # no point of one cloud on the other's table: NO_OVERLAP
    away = np.array([1, 0, 500.0, 0, 1, 0], np.float32)
    r = V.result(rm.clouds[0], rm.clouds[1], away, p)
    assert r["n_in"].tolist() == [0, 0] and r["status"] == _abi.DPG_VERIFY_NO_OVERLAP and r["n_pts"].tolist() == [360, 360]


# ------------------------------------------------------------------ host functions
def test_defaults_and_struct_layouts_match_the_header(tmp_path):
    p = _abi.default_verify_params()
    assert p.resolution == np.float32(0.1) and (p.half_cells, p.occ_radius) == (160, 2)
    assert (p.sensor[0], p.sensor[1]) == (np.float32(0.2), 0.0) and list(p.pad) == [0, 0, 0]
    sp = _abi.default_change_params()
    assert (p.sensor[0], p.sensor[1]) == (sp.laser[0], sp.laser[1])     # dpg_store_params.laser
    assert api.verify_sensor_key(p) == (2, 0) == V.sensor_key(p)
    assert lib().dpg_verify_params_check(C.byref(p)) == 0 and api.verify_params_valid(p)
    txt = open(os.path.join(INC, "dpg_slam_c.h")).read()
    sizes = {k: int(v) for k, v in re.findall(r"#define (DPG_VERIFY_\w+) (\d+)", txt)}
    assert len(re.findall(r"_Static_assert\(sizeof\(dpg_verify_params\) == DPG_VERIFY_PARAMS_SIZE && "
                          r"sizeof\(dpg_verify_result\) == DPG_VERIFY_RESULT_SIZE", txt)) == 1
    assert C.sizeof(_abi.VerifyParams) == sizes["DPG_VERIFY_PARAMS_SIZE"] == 32
    assert C.sizeof(_abi.VerifyResult) == sizes["DPG_VERIFY_RESULT_SIZE"] == 64 == _abi.VERIFY_RESULT_DTYPE.itemsize
    assert (sizes["DPG_VERIFY_OK"], sizes["DPG_VERIFY_NO_OVERLAP"]) == (_abi.DPG_VERIFY_OK, _abi.DPG_VERIFY_NO_OVERLAP) == (0, 1)
    for struct, cls in (("dpg_verify_params", _abi.VerifyParams), ("dpg_verify_result", _abi.VerifyResult)):
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
        if struct == "dpg_verify_result":   # the numpy mirror too
            assert lay[1:] == [_abi.VERIFY_RESULT_DTYPE.fields[n][1] for n in names]
    # the LDS formula of the header comment: two bit planes and the fixed part
    fixed, budget = sizes["DPG_VERIFY_LDS_FIXED"], sizes["DPG_VERIFY_LDS_BUDGET"]
    assert budget == 160 * 1024

    def formula(h):
        w = 2 * h + 1
        return 2 * (((w * w + 31) // 32 * 4 + 15) // 16 * 16) + fixed
    assert api.verify_lds_bytes(p) == formula(160) == 2 * 12896 + fixed
    assert api.verify_lds_bytes(_params(half_cells=0, sensor=(0.0, 0.0))) == 2 * 16 + fixed
    assert api.verify_lds_bytes(_params(half_cells=8)) == formula(8)


def test_parameter_errors_and_limits():
    inf, nan = float("inf"), float("nan")
    bad = [dict(resolution=0.0), dict(resolution=-0.1), dict(resolution=nan), dict(resolution=inf),
           dict(half_cells=-1), dict(occ_radius=-1), dict(occ_radius=8),
           dict(sensor=(nan, 0.0)), dict(sensor=(0.0, nan)), dict(sensor=(inf, 0.0)), dict(sensor=(0.0, -inf)),
           dict(sensor=(1e30, 0.0)), dict(half_cells=1), dict(half_cells=0)]       # the last two: the default sensor's key (2, 0) outside
    key = np.zeros(2, np.int32)
    for kw in bad:
        p = _params(**kw)
        assert lib().dpg_verify_params_check(C.byref(p)) == ERR_ARG, kw
        assert lib().dpg_verify_lds_bytes(C.byref(p)) == ERR_ARG, kw
        assert not api.verify_params_valid(p)
        with pytest.raises(_abi.DpgError):
            api.verify_lds_bytes(p)
    for kw in bad[:4] + bad[7:12]:
        assert lib().dpg_verify_sensor_key(C.byref(_params(**kw)), ptr(key, C.c_int32)) == ERR_ARG, kw
    assert lib().dpg_verify_params_check(None) == ERR_ARG and lib().dpg_verify_lds_bytes(None) == ERR_ARG
    assert lib().dpg_verify_sensor_key(None, ptr(key, C.c_int32)) == ERR_ARG
    assert lib().dpg_verify_sensor_key(C.byref(_params()), None) == ERR_ARG
    # the sensor key at +-H is accepted, at +-(H + 1) rejected, on both axes
    for H in (0, 5, 160):
        for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, -1)):
            assert api.verify_params_valid(_params(resolution=1.0, half_cells=H, sensor=(float(sx * H), float(sy * H)))), (H, sx, sy)
            q = _params(resolution=1.0, half_cells=H, sensor=(float(sx * (H + 1)), float(sy * (H + 1))))
            assert lib().dpg_verify_params_check(C.byref(q)) == ERR_ARG and lib().dpg_verify_lds_bytes(C.byref(q)) == ERR_ARG
    assert api.verify_sensor_key(_params(resolution=0.25, sensor=(0.125, -0.375))) == (1, -2)    # exact halves: away from zero
    # every limit itself
    assert api.verify_params_valid(_params(occ_radius=0)) and api.verify_params_valid(_params(occ_radius=7))
    # the LDS bytes grow with H; the largest H that fits, and the budget above it (the params stay valid)
    h, last = 2, api.verify_lds_bytes(_params(half_cells=2))
    while lib().dpg_verify_lds_bytes(C.byref(_params(half_cells=h + 1))) > 0:
        h += 1
        now = api.verify_lds_bytes(_params(half_cells=h))
        assert now >= last
        last = now
    assert last <= 160 * 1024 and h > 160
    over = _params(half_cells=h + 1)
    assert api.verify_params_valid(over) and lib().dpg_verify_lds_bytes(C.byref(over)) == ERR_ARG
    assert lib().dpg_verify_lds_bytes(C.byref(_params(half_cells=2 ** 30))) == ERR_ARG
    w = 2 * (h + 1) + 1
    assert 2 * (((w * w + 31) // 32 * 4 + 15) // 16 * 16) + 4160 > 160 * 1024


def test_verify_accept():
    r = np.zeros(7, _abi.VERIFY_RESULT_DTYPE)
    r["n_pts"] = 100
    r["n_in"] = [[100, 80]] * 7
    r["n_support"] = [[50, 40], [25, 20], [24, 40], [50, 19], [50, 40], [50, 40], [50, 40]]
    r["n_free"] = [[15, 12], [0, 0], [0, 0], [0, 0], [16, 0], [0, 13], [0, 0]]
    r["status"][6] = _abi.DPG_VERIFY_NO_OVERLAP
    assert api.verify_accept(r, 0.15, 0.25).tolist() == [True, True, False, False, False, False, False]
    assert api.verify_accept(r).tolist() == api.verify_accept(r, 0.15, 0.25).tolist()     # the defaults
    assert api.verify_accept(r, 1.0, 0.0).tolist() == [True] * 6 + [False]                 # everything but a bad status
    assert not api.verify_accept(r, -1.0, 0.0).any()                                      # nothing
    z = np.zeros(1, _abi.VERIFY_RESULT_DTYPE)
    z["status"] = _abi.DPG_VERIFY_NO_OVERLAP                                               # n_in = 0: no division by zero, rejected
    assert api.verify_accept(z, 1.0, 0.0).tolist() == [False]
    assert api.verify_accept(r[0]).shape == () and bool(api.verify_accept(r[0]))


# ------------------------------------------------------------------ the room: the reference with the oracle's ICP
def test_reference_rejects_the_converged_false_alignment_on_the_room():
    """The room of tests/csm_ref.py, 360-point clouds, the CPU oracle's ICP (downsample ratio 1,
    defaults otherwise), default verification params but the sensor at (0, 0) where the room's scans
    were taken.  From the true estimates the ICP ends millimetres from the truth; from the perturbed
    estimates it ends converged, status OK, more than a metre off -- and only the verification sees
    the difference."""
    from oracle import oracle as O
    rm = csm_ref.room()
    ip = _abi.default_icp_params()
    ip.downsample_icp_points_ratio = 1
    p = _params(sensor=(0.0, 0.0))
    tables = (V.table(rm.clouds[0], p), V.table(rm.clouds[1], p))
    out = {}
    for name, est in (("true", rm.est_true), ("perturbed", rm.est)):
        res, _, _ = O.run_icp(rm.clouds[1], rm.clouds[0], est[1], est[0], ip, O.NN_BRUTE)
        err = rm.error(res.z)[0]
        r = V.result(rm.clouds[0], rm.clouds[1], np.array(res.T, np.float32), p, tables)
        frac = r["n_free"] / np.maximum(r["n_in"], 1)
        print(f"{name}: converged {res.converged} status {res.status} iterations {res.iterations} error {err:.4f} m; "
              f"n_in {r['n_in'].tolist()} free {r['n_free'].tolist()} support {r['n_support'].tolist()}")
        out[name] = (res, err, r, frac)
    res, err, r, frac = out["true"]
    assert res.converged and res.status == _abi.DPG_ICP_OK and err < 0.05
    assert (frac <= 0.02).all() and bool(api.verify_accept(r))
    res, err, r, frac = out["perturbed"]
    assert res.converged and res.status == _abi.DPG_ICP_OK and err >= 1.0      # the premise: a converged false closure
    assert (frac >= 0.2).all() and not bool(api.verify_accept(r))


# ------------------------------------------------------------------ DpgSLAM's backend protocol
class _Backend:
    """Three nodes, one loop-closure candidate that converges; no verify method."""

    def __init__(self):
        self.calls = []

    def candidates(self, est, passes, within, across):
        return np.array([[0, 2]], np.int32)

    def icp_batch(self, clouds, edges, est, p):
        res = np.zeros(len(edges), _abi.RESULT_DTYPE)
        res["converged"] = 1
        res["status"] = _abi.DPG_ICP_OK
        res["T"] = np.arange(6 * len(edges), dtype=np.float32).reshape(-1, 6)
        self.edges = np.array(edges)
        return res

    def rebuild_graph(self, est, F):
        return est


class _Verifying(_Backend):
    def __init__(self, free):
        super().__init__()
        self.free = free

    def verify(self, clouds, edges, transforms, params, ratio):
        self.calls.append((np.array(edges), np.array(transforms), params, ratio))
        r = np.zeros(len(edges), _abi.VERIFY_RESULT_DTYPE)
        r["n_pts"], r["n_in"], r["n_support"], r["n_free"] = 100, 100, 60, self.free
        return r


def _slam(be, **kw):
    from dpgslam.slam import DpgSLAM
    s = DpgSLAM(backend=be, odometry_constraints=False, **kw)
    s.poses = np.zeros((3, 3), np.float32)
    s.node_pass = np.zeros(3, np.int32)
    return s


def test_slam_verify_option_and_the_backend_method():
    off = _slam(_Verifying(0))
    off.reoptimize()
    assert off.be.calls == [] and off.last_verify is None and "verify" not in off.last_sweep_ms
    assert off.n_factors == 1 + 2 + 1                      # the prior, two successive pairs, the closure
    vp = _abi.default_verify_params()
    s = _slam(_Backend(), loop_closure_verify=vp)
    with pytest.raises(NotImplementedError, match="loop_closure_verify needs a `verify` method on the backend"):
        s.reoptimize()
    ok = _slam(_Verifying(10), loop_closure_verify=vp)     # free 0.10 <= 0.15: kept
    ok.reoptimize()
    (edges, T, prm, ratio), = ok.be.calls
    assert edges.tolist() == [[0, 2]] and prm is vp and ratio == ok.icp_params.downsample_icp_points_ratio
    assert T.tolist() == [[12, 13, 14, 15, 16, 17]]        # the candidate's own ICP transform (edge 2 of the batch)
    assert ok.n_factors == off.n_factors and ok.factors.tobytes() == off.factors.tobytes()
    rec, ve = ok.last_verify
    assert ve.tolist() == [[0, 2]] and len(rec) == 1 and ok.last_sweep_ms["verify"] >= 0.0
    rej = _slam(_Verifying(20), loop_closure_verify=vp)    # free 0.20 > 0.15: dropped, the successive pairs stay
    rej.reoptimize()
    assert rej.n_factors == off.n_factors - 1 and rej.factors.tobytes() == off.factors[:-1].tobytes()
    lax = _slam(_Verifying(20), loop_closure_verify=vp, verify_max_free_fraction=0.2)
    lax.reoptimize()
    assert lax.n_factors == off.n_factors
