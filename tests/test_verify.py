"""Loop-closure verification on the GPU (csrc/dpg_verify.hip) against the numpy restatement
tests/verify_ref.py: table bytes and result records are equal, no tolerance (after one float
transform per point all of it is integer).  Then batches, order-freedom, the errors, the end-to-end
case the feature exists for -- an ICP that converges more than a metre off and is rejected -- and
DpgSLAM's loop_closure_verify option."""
import ctypes as C

import numpy as np
import pytest

import csm_ref
import verify_ref as V
from dpgslam import _abi, api
from dpgslam._abi import lib, ptr, vptr

pytestmark = pytest.mark.gpu

KT = 256        # the kernel's workgroup size: moving points per sweep
KCHUNK = 512    # model points per LDS chunk of the kernel: a cloud above it takes the chunk loop again
IDENT = np.array([1, 0, 0, 0, 1, 0], np.float32)


def _params(**kw):
    p = _abi.default_verify_params()
    for k, v in kw.items():
        if k == "sensor":
            p.sensor[0], p.sensor[1] = v
        else:
            setattr(p, k, v)
    return p


def _upload(ctx, clouds, ratio=1):
    clouds = [np.ascontiguousarray(c, np.float32).reshape(-1, 2) for c in clouds]
    offs = np.zeros(len(clouds) + 1, np.int64)
    offs[1:] = np.cumsum([len(c) for c in clouds])
    pts = np.concatenate(clouds) if offs[-1] else np.zeros((0, 2), np.float32)
    ctx.upload_scans(np.ascontiguousarray(pts, np.float32), offs, ratio)
    return clouds


def _largest_half_cells(**kw):
    h = 2
    while lib().dpg_verify_lds_bytes(C.byref(_params(half_cells=h + 1, **kw))) > 0:
        h += 1
    return h


def _check_tables(ctx, clouds, p):
    for v, c in enumerate(clouds):
        got = ctx.verify_table(v, p)
        want = V.table(c, p)
        assert got.shape == want.shape
        np.testing.assert_array_equal(got, want, err_msg=f"node {v}")


# ------------------------------------------------------------------ table bytes
def test_table_config1_nodes(ctx, workload):
    w = workload("config1")
    ctx.upload_scans(w.pts, w.offsets, 5)   # the table is built over the store's downsampled clouds
    p = _params()                           # the default sensor: where scan_to_cloud puts the lidar
    for v in range(w.V):
        got = ctx.verify_table(v, p)
        np.testing.assert_array_equal(got, V.table(api.downsample(w.cloud(v), 5), p))
        assert got.max() == 2 and np.count_nonzero(got == 1) > 0 and np.count_nonzero(got == 0) > 0
    assert ctx.verify_kernel_ms() > 0.0


def _edge_cloud(p, rng, n):
    """Points around, on and beyond the table's edge: keys up to H + R + 2 on both axes, both signs."""
    lim = (p.half_cells + p.occ_radius + 2.4) * p.resolution
    return rng.uniform(-lim, lim, (n, 2)).astype(np.float32)


def _table_cases():
    rng = np.random.default_rng(12)
    big = np.float32(3e9)
    half = np.array([[x, y] for x in (0.125, 0.375, -0.125, -0.375, 0.625, -0.625) for y in (0.125, -0.125, -0.875, 0.875)],
                    np.float32)   # exact halves of a 0.25 m cell, both signs
    corners = [[2.0, 2.0], [-2.0, 2.04], [2.0, -2.0], [-2.0, -2.0], [2.1, 2.1], [-2.1, 2.1], [2.3, 0.0], [2.34, -2.3],
               [2.4, 0.0], [0.0, -2.36], [1.9, -1.9], [0.0, 2.0], [-2.0, 0.0]]
    h = _largest_half_cells()
    cases = {
        "single_point": (_params(half_cells=12), [[[0.31, -0.52]]]),
        "duplicates": (_params(half_cells=12), [np.tile(np.array([[0.31, -0.52], [-1.0, 1.0]], np.float32), (40, 1))]),
        "empty_cloud": (_params(half_cells=12), [[[0.5, 0.1]], np.zeros((0, 2), np.float32), [[-0.4, 0.9]]]),
        "edge_and_beyond": (_params(half_cells=20), [_edge_cloud(_params(half_cells=20), rng, 150), corners]),
        # 5.3e7 m is key 5.3e8 < 2^29: a valid far point, the 64-bit steps; 3e9 m counts for nothing
        "non_finite_and_huge": (_params(half_cells=12), [[[np.nan, 0.0], [0.0, np.inf], [-np.inf, np.nan], [big, 0.0],
                                                          [0.0, -big], [5.3e7, 0.0], [0.5, 0.5], [-5.3e7, 2.9e7], [1e6, -5.3e7]]]),
        # 2 (2H + 1) n against 2^31 - 1 at H = 12: n = 42949672 is the last 32-bit ray, 42949676 the first 64-bit one
        "step_width_threshold": (_params(half_cells=12, resolution=1.0, sensor=(0.0, 0.0)),
                                 [[[42949672.0, 1e6]], [[42949676.0, -3e6]], [[2e6, -42949672.0], [-7.0, 42949676.0]]]),
        "half_cell_boundaries": (_params(half_cells=10, resolution=0.25, occ_radius=0), [half, -half, 3 * half]),
        "sensor_cell": (_params(half_cells=12, occ_radius=0), [[[0.2, 0.0]], [[0.24, 0.04], [0.16, -0.049], [0.3, 0.0]], [[0.2, 0.0], [1.0, 0.5]]]),
        "sensor_off_origin": (_params(half_cells=20, sensor=(-0.73, 1.18)), [_edge_cloud(_params(half_cells=20), rng, 300)]),
        "sensor_at_plus_h": (_params(half_cells=20, sensor=(2.0, 2.0)), [_edge_cloud(_params(half_cells=20), rng, 300)]),
        "sensor_at_minus_h": (_params(half_cells=20, sensor=(-2.0, 2.0)), [_edge_cloud(_params(half_cells=20), rng, 300), [[60.0, 2.0]]]),
        "radius_0": (_params(half_cells=20, occ_radius=0), [_edge_cloud(_params(half_cells=20, occ_radius=0), rng, 500)]),
        "radius_7": (_params(half_cells=20, occ_radius=7), [_edge_cloud(_params(half_cells=20, occ_radius=7), rng, 12), [[0.0, 0.0]]]),
        "half_cells_0": (_params(half_cells=0, sensor=(0.0, 0.0)), [[[0.0, 0.0], [0.2, 0.0]], [[0.31, 0.0]], [[0.04, -0.04]]]),
        "half_cells_8": (_params(half_cells=8), [_edge_cloud(_params(half_cells=8), rng, 12)]),
        "chunk_plus_1": (_params(half_cells=30, occ_radius=0), [_edge_cloud(_params(half_cells=30), rng, KCHUNK + 1),
                                                                 _edge_cloud(_params(half_cells=30), rng, KCHUNK - 1)]),
        "cloud_16384": (_params(half_cells=200, occ_radius=0), [_edge_cloud(_params(half_cells=200), rng, 16384)]),
        "largest_half_cells": (_params(half_cells=h), [_edge_cloud(_params(half_cells=h), rng, 1500)]),
    }
    return cases


_TABLE_CASES = None


@pytest.mark.parametrize("name", ["single_point", "duplicates", "empty_cloud", "edge_and_beyond", "non_finite_and_huge",
                                  "step_width_threshold", "half_cell_boundaries", "sensor_cell", "sensor_off_origin",
                                  "sensor_at_plus_h", "sensor_at_minus_h", "radius_0", "radius_7", "half_cells_0",
                                  "half_cells_8", "chunk_plus_1", "cloud_16384", "largest_half_cells"])
def test_table_bytes_equal_the_reference(ctx, name):
    global _TABLE_CASES
    if _TABLE_CASES is None:
        _TABLE_CASES = _table_cases()
    p, clouds = _TABLE_CASES[name]
    if name.startswith("sensor_at"):
        assert max(abs(k) for k in V.sensor_key(p)) == p.half_cells
    if name == "largest_half_cells":
        assert lib().dpg_verify_lds_bytes(C.byref(p)) > 64 * 1024
        assert lib().dpg_verify_lds_bytes(C.byref(_params(half_cells=p.half_cells + 1))) < 0
    _check_tables(ctx, _upload(ctx, clouds), p)


# ------------------------------------------------------------------ records
SIZES = [0, 1, 63, 64, 65, KT - 1, KT, KT + 1, KCHUNK - 1, KCHUNK + 1, 2 * KCHUNK + 4]
_ICP = {}


def _room_icp(which):
    """The CPU oracle's ICP on the room (ratio 1) from the true / the perturbed estimates: (result, error in m)."""
    if which not in _ICP:
        from oracle import oracle as O
        rm = csm_ref.room()
        ip = _abi.default_icp_params()
        ip.downsample_icp_points_ratio = 1
        est = rm.est_true if which == "true" else rm.est
        res, _, _ = O.run_icp(rm.clouds[1], rm.clouds[0], est[1], est[0], ip, O.NN_BRUTE)
        _ICP[which] = (res, rm.error(res.z)[0])
    return _ICP[which]


def _transforms():
    rm = csm_ref.room()
    nan = IDENT.copy()
    nan[2] = np.nan
    nan_c = csm_ref.guess_of(*rm.truth)
    nan_c[0] = np.nan
    return {"true": csm_ref.guess_of(*rm.truth), "false_icp": np.array(_room_icp("perturbed")[0].T, np.float32),
            "identity": IDENT, "off_the_table": np.array([1, 0, 500.0, 0, 1, -40.0], np.float32), "nan_t": nan, "nan_c": nan_c}


def test_records_equal_the_reference(ctx):
    """Node 0: the room's target scan; node 1 + k: SIZES[k] points drawn from the room's source scan."""
    rm = csm_ref.room()
    rng = np.random.default_rng(5)
    srcs = [(rm.clouds[1][rng.integers(0, len(rm.clouds[1]), n)] + rng.normal(0, 0.03, (n, 2))).astype(np.float32) for n in SIZES]
    clouds = _upload(ctx, [rm.clouds[0]] + srcs)
    p = _params(sensor=(0.0, 0.0))          # the room's scans are taken from the body origin
    tables = [V.table(c, p) for c in clouds]
    assert _room_icp("perturbed")[1] >= 1.0
    for name, T in _transforms().items():
        edges = np.array([[0, 1 + k] for k in range(len(SIZES))], np.int32)
        got = ctx.verify_batch(edges, np.tile(T, (len(edges), 1)), p)
        for k, n in enumerate(SIZES):
            want = V.result(clouds[0], clouds[1 + k], T, p, (tables[0], tables[1 + k]))
            assert got[k].tobytes() == want.tobytes(), (name, n, got[k], want)
        if name in ("off_the_table", "nan_t", "nan_c"):
            assert (got["status"] == _abi.DPG_VERIFY_NO_OVERLAP).all() and not got["n_in"].any()
        elif name == "true":
            assert (got["status"][1:] == _abi.DPG_VERIFY_OK).all() and got["status"][0] == _abi.DPG_VERIFY_NO_OVERLAP
        assert got["n_pts"][:, 0].tolist() == SIZES and (got["n_pts"][:, 1] == 360).all()


# ------------------------------------------------------------------ batches
def _batch_store(ctx):
    rm = csm_ref.room()
    rng = np.random.default_rng(21)
    clouds = [rm.clouds[0], rm.clouds[1], np.zeros((0, 2), np.float32), [[0.0, 0.0]],
              (rm.clouds[1][rng.integers(0, 360, KT + 1)] + rng.normal(0, 0.02, (KT + 1, 2))).astype(np.float32),
              (rm.clouds[0][rng.integers(0, 360, KCHUNK + 1)] + rng.normal(0, 0.02, (KCHUNK + 1, 2))).astype(np.float32)]
    return rm, _upload(ctx, clouds)


def _batch(rm, n):
    g = csm_ref.guess_of
    base = [(0, 1, g(*rm.truth)),
            (0, 0, g(0.1, 0.1, 0.01)),                   # source = target
            (2, 1, g(0, 0, 0)),                          # empty target
            (0, 2, g(0.5, 0.5, 0.5)),                    # empty source
            (0, 4, g(rm.truth[0] - 0.4, rm.truth[1], rm.truth[2] - 0.02)),   # the target repeated
            (5, 4, g(rm.truth[0], rm.truth[1] + 0.2, rm.truth[2])),
            (2, 2, g(0, 0, 0)),                          # both empty
            (4, 5, g(-rm.truth[0], -rm.truth[1], -rm.truth[2])),
            (3, 0, g(1.0, -2.0, 3.0)),
            (1, 0, g(0, 0, 0))]
    rng = np.random.default_rng(n)
    out = []
    for e in range(n):
        t, s, T = base[e % len(base)]
        if e >= len(base):   # the same pairs again under other transforms
            x, y, th = csm_ref.guess_pose(T)
            T = g(x + rng.uniform(-0.5, 0.5), y + rng.uniform(-0.5, 0.5), th + rng.uniform(-0.2, 0.2))
        out.append((t, s, T))
    return out


@pytest.mark.parametrize("n", [1, 3, 257])
def test_batches_equal_the_reference(ctx, n):
    rm, clouds = _batch_store(ctx)
    p = _params(half_cells=100, sensor=(0.0, 0.0))
    pairs = _batch(rm, n)
    edges = np.array([(t, s) for t, s, _ in pairs], np.int32)
    Ts = np.stack([T for _, _, T in pairs])
    out = ctx.verify_batch(edges, Ts, p)
    again = ctx.verify_batch(edges, Ts, p)
    assert out.tobytes() == again.tobytes()
    tables = [V.table(c, p) for c in clouds]
    for e, (t, s, T) in enumerate(pairs):
        want = V.result(clouds[t], clouds[s], T, p, (tables[t], tables[s]))
        assert out[e].tobytes() == want.tobytes(), (e, t, s, out[e], want)
    assert out["status"][0] == _abi.DPG_VERIFY_OK and out["n_support"][0].min() > 300
    if n == 257:
        assert (out["status"][[2, 3, 6]] == _abi.DPG_VERIFY_NO_OVERLAP).all()
        assert out["n_support"][1].tolist() != [360, 360]                     # t = s, but not under the identity
        assert len({r["n_free"].tobytes() + r["n_support"].tobytes() for r in out[0::10]}) > 5   # the repeated pair: other transforms, other counts


def test_point_order_does_not_matter(ctx):
    rm, clouds = _batch_store(ctx)
    p = _params(half_cells=100, sensor=(0.0, 0.0))
    pairs = _batch(rm, 25)
    edges = np.array([(t, s) for t, s, _ in pairs], np.int32)
    Ts = np.stack([T for _, _, T in pairs])
    out = ctx.verify_batch(edges, Ts, p)
    tbl = [ctx.verify_table(v, p) for v in range(len(clouds))]
    rng = np.random.default_rng(4)
    _upload(ctx, [c[rng.permutation(len(c))] for c in clouds])
    assert ctx.verify_batch(edges, Ts, p).tobytes() == out.tobytes()
    for v in range(len(clouds)):
        np.testing.assert_array_equal(ctx.verify_table(v, p), tbl[v])


# ------------------------------------------------------------------ errors
def test_errors(ctx):
    rm, clouds = _batch_store(ctx)
    p = _params(half_cells=100, sensor=(0.0, 0.0))
    edges = np.array([[0, 1], [0, 4]], np.int32)
    T = np.stack([IDENT] * 2)
    with pytest.raises(_abi.DpgError, match=r"\(-1\)"):                      # the LDS budget
        ctx.verify_batch(edges, T, _params(half_cells=_largest_half_cells() + 1))
    with pytest.raises(_abi.DpgError, match=r"\(-1\)"):
        ctx.verify_table(0, _params(occ_radius=8))
    with pytest.raises(_abi.DpgError, match=r"\(-1\)"):                      # the sensor outside the table
        ctx.verify_batch(edges, T, _params(half_cells=1))
    with pytest.raises(_abi.DpgError, match=r"\(-1\)"):
        ctx.verify_batch(edges, T, _params(resolution=float("nan")))
    out = np.zeros(2, _abi.VERIFY_RESULT_DTYPE)                              # cap too small: nothing written
    out.view(np.uint8)[:] = 7
    before = out.tobytes()
    rc = lib().dpg_verify_batch(ctx.handle, ptr(edges, C.c_int32), 2, ptr(T, C.c_float), C.byref(p), vptr(out), 1)
    assert rc == -4 and out.tobytes() == before
    tb = np.zeros(10, np.uint8)
    assert lib().dpg_verify_table(ctx.handle, 0, C.byref(p), ptr(tb, C.c_uint8), tb.size) == -4 and not tb.any()
    for bad in ([[0, len(clouds)]], [[-1, 0]], [[len(clouds), 0]]):          # a bad edge: nothing written either
        with pytest.raises(_abi.DpgError, match=r"\(-1\)"):
            ctx.verify_batch(np.array(bad, np.int32), T[:1], p)
        e2 = np.array([[0, 1]] + bad, np.int32)
        assert lib().dpg_verify_batch(ctx.handle, ptr(e2, C.c_int32), 2, ptr(T, C.c_float), C.byref(p), vptr(out), 2) == -1
        assert out.tobytes() == before
    with pytest.raises(_abi.DpgError, match=r"\(-1\)"):
        ctx.verify_table(len(clouds), p)
    with pytest.raises(ValueError):
        ctx.verify_batch(edges, T[:1], p)
    assert len(ctx.verify_batch(np.zeros((0, 2), np.int32), np.zeros((0, 6), np.float32), p)) == 0   # n_edges = 0
    with api.Context(0) as fresh:                                            # no scans uploaded
        assert fresh.verify_kernel_ms() < 0
        with pytest.raises(_abi.DpgError, match=r"\(-3\)"):
            fresh.verify_batch(edges, T, p)
        with pytest.raises(_abi.DpgError, match=r"\(-3\)"):
            fresh.verify_table(0, p)
    with api.Context(0, virtual=2) as multi:                                 # a multi-device form
        multi.upload_scans(np.concatenate(clouds[:2]), np.array([0, 360, 720], np.int64), 1)
        for call in (lambda: multi.verify_batch(edges[:1], T[:1], p), lambda: multi.verify_table(0, p)):
            with pytest.raises(_abi.DpgError, match=r"\(-3\)"):
                call()


# ------------------------------------------------------------------ end to end
def test_end_to_end_converged_false_closure_is_rejected(ctx):
    """Two scans of the room (csm_ref.Room), the source's estimate off by (-1.3 m, 1.2 m, -0.16 rad).
    ICP from those estimates (ratio 1, defaults otherwise) converges with status OK at least a metre
    from the truth (1.376 m on the CPU oracle); its transform shows free-space fractions of 83 / 360
    and 98 / 360 in the reference and is rejected at the default thresholds.  ICP from the true
    estimates (0.0019 m off; 3 / 360 and 0 / 360) is accepted."""
    rm = csm_ref.room()
    _upload(ctx, rm.clouds)
    ip = _abi.default_icp_params()
    ip.downsample_icp_points_ratio = 1
    edges = np.array([[0, 1]], np.int32)
    p = _params(sensor=(0.0, 0.0))
    for name, est, accept in (("perturbed", rm.est, False), ("true", rm.est_true, True)):
        res, _ = ctx.icp_batch(edges, est, ip, compute_cov=False)
        err = rm.error(res["z"][0])[0]
        rec = ctx.verify_batch(edges, res["T"], p)
        want = V.result(rm.clouds[0], rm.clouds[1], res["T"][0], p)
        print(f"{name}: ICP converged {int(res['converged'][0])} status {int(res['status'][0])} error {err:.4f} m; n_in "
              f"{rec['n_in'][0].tolist()} free {rec['n_free'][0].tolist()} support {rec['n_support'][0].tolist()}; "
              f"kernel {ctx.verify_kernel_ms():.3f} ms")
        assert res["converged"][0] and res["status"][0] == _abi.DPG_ICP_OK
        assert err >= 1.0 if name == "perturbed" else err < 0.05
        assert rec[0].tobytes() == want.tobytes()
        assert bool(api.verify_accept(rec)[0]) is accept


def test_other_batches_are_untouched(ctx):
    rm = csm_ref.room()
    _upload(ctx, rm.clouds)
    ip = _abi.default_icp_params()
    ip.downsample_icp_points_ratio = 1
    edges = np.array([[0, 1], [1, 0]], np.int32)
    est = np.array([[0, 0, 0], [rm.truth[0] + 0.1, rm.truth[1] - 0.1, rm.truth[2]]], np.float32)
    cp = _abi.default_csm_params()
    m0 = ctx.csm_batch(edges, poses=est, params=cp)
    r0, _ = ctx.icp_batch(edges, est, ip, compute_cov=False)
    v0 = ctx.verify_batch(edges, r0["T"], _params(sensor=(0.0, 0.0)))
    assert (v0["status"] == _abi.DPG_VERIFY_OK).all()
    assert ctx.csm_batch(edges, poses=est, params=cp).tobytes() == m0.tobytes()
    r1, _ = ctx.icp_batch(edges, est, ip, compute_cov=False)
    assert r1.tobytes() == r0.tobytes()
    assert ctx.verify_batch(edges, r0["T"], _params(sensor=(0.0, 0.0))).tobytes() == v0.tobytes()


# ------------------------------------------------------------------ DpgSLAM plumbing
def _drive_two_passes(slam, w):
    rng = np.random.default_rng(3)
    for ps in range(len(w.pass_start) - 1):
        if ps:
            slam.incrementPassNumber()
        for v in range(int(w.pass_start[ps]), int(w.pass_start[ps + 1])):
            odom = w.est[v].astype(np.float64) + rng.normal(0, [0.01, 0.01, 0.002])
            slam.ObserveOdometry(odom[:2].astype(np.float32), np.float32(odom[2]))
            slam.ObserveLaser(w.ranges[v], 0.0, float(w.geom[v, 2]), float(w.geom[v, 0]), float(w.geom[v, 1]))
    slam.reoptimize()   # a sweep over both passes: its loop closures are what the runs below compare


def test_slam_verify_option():
    from dpgslam import synth
    from dpgslam.slam import DpgSLAM, GpuBackend

    class Recording(GpuBackend):
        def icp_batch(self, clouds, edges, est, p):
            r = super().icp_batch(clouds, edges, est, p)
            self.rec_icp = (np.array(edges), r.copy())
            return r

        def icp_batch_guess(self, clouds, edges, guesses, n_nodes, p):
            r = super().icp_batch_guess(clouds, edges, guesses, n_nodes, p)
            self.rec_icp = (np.array(edges), r.copy())
            return r

        def verify(self, clouds, edges, transforms, params, ratio):
            self.rec_verify = (np.array(edges), np.array(transforms))
            return super().verify(clouds, edges, transforms, params, ratio)

    w = synth.make_dynamic(n_passes=2, nodes_per_pass=8, n_beams=360, world_size=16.0, range_max=8.0, n_boxes=6, seed=9)
    vp = _abi.default_verify_params()
    runs = {}
    for name, kw in (("off", {}),
                     ("all", dict(loop_closure_verify=vp, verify_max_free_fraction=1.0, verify_min_support_fraction=0.0)),
                     ("none", dict(loop_closure_verify=vp, verify_max_free_fraction=-1.0, verify_min_support_fraction=0.0)),
                     ("prematch", dict(loop_closure_verify=vp, verify_max_free_fraction=1.0, verify_min_support_fraction=0.0,
                                       loop_closure_prematch=_abi.default_csm_params(), prematch_min_response=1.5))):
        with api.Context(0) as c:
            be = Recording(c)
            s = DpgSLAM(backend=be, **kw)
            _drive_two_passes(s, w)
            V_ = len(s.poses)
            edges, res = be.rec_icp
            conv = (res["converged"][V_ - 1:] != 0) & (res["status"][V_ - 1:] == _abi.DPG_ICP_OK)
            runs[name] = (s.factors.tobytes(), s.poses.tobytes(), s.n_factors, int(conv.sum()))
            if name == "off":
                assert s.last_verify is None and not hasattr(be, "rec_verify") and "verify" not in s.last_sweep_ms
                assert conv.sum() > 0
                continue
            rec, ve = s.last_verify
            ve_rec, T_rec = be.rec_verify
            assert np.array_equal(ve, ve_rec) and np.array_equal(ve, edges[V_ - 1:][conv]) and len(rec) == len(ve) > 0
            assert T_rec.tobytes() == res["T"][V_ - 1:][conv].tobytes()          # that ICP's own transforms
            assert c.verify_batch(ve_rec, T_rec, vp).tobytes() == rec.tobytes()   # the kernel called by hand
            assert s.last_sweep_ms["verify"] > 0.0
            if name == "all":
                frac_free = rec["n_free"] / np.maximum(rec["n_in"], 1)
                frac_sup = rec["n_support"] / np.maximum(rec["n_in"], 1)
                rejected = int((~api.verify_accept(rec)).sum())
                print(f"{len(rec)} converged closures: free fraction max {frac_free.max():.3f} median {np.median(frac_free):.3f}, "
                      f"support fraction min {frac_sup.min():.3f}; the default thresholds reject {rejected}")
    assert runs["all"][:3] == runs["off"][:3]                                    # accept everything: today's bytes
    assert runs["prematch"][:3] == runs["off"][:3]                               # a matcher that is never taken, then accept everything
    assert runs["none"][2] == runs["off"][2] - runs["off"][3]                    # every loop closure dropped, nothing else
