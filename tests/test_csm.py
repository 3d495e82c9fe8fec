"""Correlative scan matching on the GPU (csrc/dpg_csm.hip) against the numpy restatement
tests/csm_ref.py: table bytes, full score volumes and result records are equal, no tolerance (after
one float transform per point and angle all of it is integer).  Then the errors, ICP from explicit
guesses against ICP from poses, the end-to-end case the feature exists for -- a guess outside ICP's
basin that the matcher brings back -- and DpgSLAM's loop_closure_prematch option."""
import ctypes as C
import math

import numpy as np
import pytest

import csm_ref as R
from dpgslam import _abi, api
from dpgslam._abi import lib, ptr, vptr

pytestmark = pytest.mark.gpu

KT = 1024       # the kernel's workgroup size: shifts per sweep of the window
KCHUNK = 2048   # points per LDS chunk of the kernel: a cloud above it takes the chunk loop again


def _params(**kw):
    p = _abi.default_csm_params()
    for k, v in kw.items():
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
    h = 0
    while lib().dpg_csm_lds_bytes(C.byref(_params(half_cells=h + 1, **kw))) > 0:
        h += 1
    return h


def _check_tables(ctx, clouds, p):
    for v, c in enumerate(clouds):
        got = ctx.csm_table(v, p)
        want = R.table(c, p)
        assert got.shape == want.shape
        np.testing.assert_array_equal(got, want, err_msg=f"node {v}")


# ------------------------------------------------------------------ table bytes
def test_table_config1_nodes(ctx, workload):
    w = workload("config1")
    ctx.upload_scans(w.pts, w.offsets, 5)   # the table is built over the store's downsampled clouds
    p = _params()
    ds = [api.downsample(w.cloud(v), 5) for v in range(w.V)]
    for v in range(w.V):
        got = ctx.csm_table(v, p)
        np.testing.assert_array_equal(got, R.table(ds[v], p))
        assert got.max() == 255 and 0 < np.count_nonzero(got) < got.size
    assert ctx.csm_kernel_ms() > 0.0


def _edge_cloud(p, rng, n):
    """Points around, on and beyond the table's edge: keys up to H + R + 2 on both axes, both signs."""
    lim = (p.half_cells + p.kernel_radius + 2.4) * p.resolution
    return rng.uniform(-lim, lim, (n, 2)).astype(np.float32)


def _table_cases():
    rng = np.random.default_rng(11)
    big = np.float32(3e9)
    half = np.array([[x, y] for x in (0.125, 0.375, -0.125, -0.375, 0.625, -0.625) for y in (0.125, -0.125, -0.875, 0.875)],
                    np.float32)   # exact halves of a 0.25 m cell, both signs
    cases = {
        "single_point": (_params(half_cells=12), [[[0.31, -0.52]]]),
        "duplicates": (_params(half_cells=12), [np.tile(np.array([[0.31, -0.52], [-1.0, 1.0]], np.float32), (40, 1))]),
        "empty_cloud": (_params(half_cells=12), [np.zeros((0, 2), np.float32), [[0.1, 0.1]], np.zeros((0, 2), np.float32)]),
        "edge_and_beyond": (_params(half_cells=20), [_edge_cloud(_params(half_cells=20), rng, 3000),
                                                     [[2.0, 2.0], [-2.0, 2.04], [2.3, 0.0], [2.34, -2.3], [2.4, 0.0], [0.0, -2.36]]]),
        "non_finite_and_huge": (_params(half_cells=12), [[[np.nan, 0.0], [0.0, np.inf], [-np.inf, np.nan], [big, 0.0],
                                                          [0.0, -big], [5.3e7, 0.0], [0.5, 0.5]]]),
        "half_cell_boundaries": (_params(half_cells=10, resolution=0.25, sigma=0.25), [half, -half]),
        "radius_0": (_params(half_cells=20, kernel_radius=0), [_edge_cloud(_params(half_cells=20, kernel_radius=0), rng, 500)]),
        "radius_7": (_params(half_cells=20, kernel_radius=7, sigma=0.3), [_edge_cloud(_params(half_cells=20, kernel_radius=7), rng, 500),
                                                                         [[0.0, 0.0]]]),
        "radius_7_lut_zeros": (_params(half_cells=20, kernel_radius=7, sigma=0.1), [_edge_cloud(_params(half_cells=20, kernel_radius=7), rng, 300)]),
        "half_cells_0": (_params(half_cells=0), [[[0.0, 0.0], [0.2, 0.0]], [[0.31, 0.0]]]),
        "half_cells_8": (_params(half_cells=8), [_edge_cloud(_params(half_cells=8), rng, 200)]),
        "chunk_plus_1": (_params(half_cells=30), [_edge_cloud(_params(half_cells=30), rng, KCHUNK + 1),
                                                  _edge_cloud(_params(half_cells=30), rng, KCHUNK - 1)]),
        "cloud_16384": (_params(half_cells=60), [_edge_cloud(_params(half_cells=60), rng, 16384)]),
    }
    h = _largest_half_cells()
    cases["largest_half_cells"] = (_params(half_cells=h), [_edge_cloud(_params(half_cells=h), rng, 1500)])
    h0 = _largest_half_cells(half_x=0, half_y=0, half_a=0)
    cases["largest_half_cells_no_window"] = (_params(half_cells=h0, half_x=0, half_y=0, half_a=0),
                                             [_edge_cloud(_params(half_cells=h0), rng, 1500)])
    return cases


_TABLE_CASES = None


@pytest.mark.parametrize("name", ["single_point", "duplicates", "empty_cloud", "edge_and_beyond", "non_finite_and_huge",
                                  "half_cell_boundaries", "radius_0", "radius_7", "radius_7_lut_zeros", "half_cells_0",
                                  "half_cells_8", "chunk_plus_1", "cloud_16384", "largest_half_cells",
                                  "largest_half_cells_no_window"])
def test_table_bytes_equal_the_reference(ctx, name):
    global _TABLE_CASES
    if _TABLE_CASES is None:
        _TABLE_CASES = _table_cases()
    p, clouds = _TABLE_CASES[name]
    if name.startswith("largest"):
        assert lib().dpg_csm_lds_bytes(C.byref(p)) > 0
        q = _params(half_cells=p.half_cells + 1, half_x=p.half_x, half_y=p.half_y, half_a=p.half_a)
        assert lib().dpg_csm_lds_bytes(C.byref(q)) < 0
    _check_tables(ctx, _upload(ctx, clouds), p)


# ------------------------------------------------------------------ score volumes
SIZES = [0, 1, 63, 64, 65, KT - 1, KT, KT + 1, KCHUNK - 1, KCHUNK + 1, 2 * KCHUNK + 4]
WINDOWS = {"w000": (0, 0, 0), "w102": (1, 0, 2), "w371": (3, 7, 1), "w_above_kt": (20, 20, 1), "w_wide": (64, 3, 0)}


def _score_store(ctx):
    """Node 0: the room's target scan; node 1 + k: SIZES[k] points drawn from the room's source scan."""
    rm = R.room()
    rng = np.random.default_rng(5)
    srcs = [(rm.clouds[1][rng.integers(0, len(rm.clouds[1]), n)] + rng.normal(0, 0.03, (n, 2))).astype(np.float32) for n in SIZES]
    return rm, _upload(ctx, [rm.clouds[0]] + srcs)


def test_score_volumes_equal_the_reference(ctx):
    rm, clouds = _score_store(ctx)
    g = R.guess_of(rm.truth[0] + 0.18, rm.truth[1] - 0.12, rm.truth[2] + 0.01)
    shifts = set()
    for wname, (hx, hy, ha) in WINDOWS.items():
        p = _params(half_cells=100, half_x=hx, half_y=hy, half_a=ha)
        shifts.add((2 * hx + 1) * (2 * hy + 1))
        T = R.table(clouds[0], p)
        for k, n in enumerate(SIZES):
            got = ctx.csm_scores(0, 1 + k, g, p)
            want = R.scores(T, clouds[1 + k], g, p)
            np.testing.assert_array_equal(got, want, err_msg=f"{wname} n_src {n}")
            assert n == 0 or got.max() > 0
    assert min(shifts) < KT < max(shifts)   # one sweep of the window, and more than one


@pytest.mark.parametrize("k", [0, 4, 7])   # 0, 65 and KT + 1 points
def test_score_volume_default_window(ctx, k):
    rm, clouds = _score_store(ctx)
    p = _params()
    assert (2 * p.half_x + 1) * (2 * p.half_y + 1) == 961
    g = api.icp_guess(rm.est[1], rm.est[0])
    got = ctx.csm_scores(0, 1 + k, g, p)
    np.testing.assert_array_equal(got, R.scores(R.table(clouds[0], p), clouds[1 + k], g, p))
    assert got.shape == (41, 31, 31)


def test_score_volume_points_leaving_the_table(ctx):
    """A small table under a wide window: most shifted cells fall outside it, and source points lie
    up to and beyond the window away from the table's edge (the kernel drops those, exactly)."""
    rng = np.random.default_rng(8)
    p = _params(half_cells=6, half_x=9, half_y=4, half_a=2, angle_step=0.2)
    tgt = rng.uniform(-0.9, 0.9, (60, 2)).astype(np.float32)
    src = rng.uniform(-2.6, 2.6, (700, 2)).astype(np.float32)
    src[:4] = [[np.nan, 0], [0, np.inf], [4e9, 0], [6e7, 0.0]]
    clouds = _upload(ctx, [tgt, src])
    for g in (R.guess_of(0, 0, 0), R.guess_of(0.43, -0.27, 2.9), R.guess_of(-1.5, 0.35, -1.2)):
        np.testing.assert_array_equal(ctx.csm_scores(0, 1, g, p), R.scores(R.table(tgt, p), clouds[1], g, p))


# ------------------------------------------------------------------ batches
def _batch_store(ctx):
    rm = R.room()
    rng = np.random.default_rng(21)
    clouds = [rm.clouds[0], rm.clouds[1], np.zeros((0, 2), np.float32), [[0.0, 0.0]],
              (rm.clouds[1][rng.integers(0, 360, KT + 1)] + rng.normal(0, 0.02, (KT + 1, 2))).astype(np.float32),
              (rm.clouds[0][rng.integers(0, 360, KCHUNK + 1)] + rng.normal(0, 0.02, (KCHUNK + 1, 2))).astype(np.float32),
              [[-0.2, 0.0], [0.2, 0.0]]]     # node 6 under node 3 as source: score 255 at dx = -2 and dx = +2
    return rm, _upload(ctx, clouds)


def _batch(rm, n):
    base = [(0, 1, R.guess_of(rm.truth[0] + 0.3, rm.truth[1] - 0.2, rm.truth[2] + 0.02)),
            (6, 3, R.guess_of(0, 0, 0)),                  # the constructed tie
            (0, 0, R.guess_of(0.1, 0.1, 0.01)),           # source = target
            (2, 1, R.guess_of(0, 0, 0)),                  # empty target
            (0, 2, R.guess_of(0.5, 0.5, 0.5)),            # empty source
            (0, 4, R.guess_of(rm.truth[0] - 0.4, rm.truth[1], rm.truth[2] - 0.02)),   # the target repeated
            (4, 5, R.guess_of(-rm.truth[0], -rm.truth[1], -rm.truth[2])),
            (5, 4, R.guess_of(rm.truth[0], rm.truth[1] + 0.2, rm.truth[2])),
            (2, 2, R.guess_of(0, 0, 0)),                  # both empty
            (3, 6, R.guess_of(0, 0, 0))]
    rng = np.random.default_rng(n)
    out = []
    for e in range(n):
        t, s, g = base[e % len(base)]
        if e >= len(base):   # the same pairs again from other guesses
            x, y, th = R.guess_pose(g)
            g = R.guess_of(x + rng.uniform(-0.3, 0.3), y + rng.uniform(-0.3, 0.3), th + rng.uniform(-0.03, 0.03))
        out.append((t, s, g))
    if n == 1:
        out = [base[0]]
    return out


@pytest.mark.parametrize("n", [1, 3, 257])
def test_batches_equal_the_reference(ctx, n):
    rm, clouds = _batch_store(ctx)
    p = _params(half_cells=100, half_x=5, half_y=4, half_a=3)
    pairs = _batch(rm, n)
    edges = np.array([(t, s) for t, s, _ in pairs], np.int32)
    guesses = np.stack([g for _, _, g in pairs])
    out = ctx.csm_batch(edges, guesses=guesses, params=p)
    again = ctx.csm_batch(edges, guesses=guesses, params=p)
    assert out.tobytes() == again.tobytes()
    tables = {}
    for e, (t, s, g) in enumerate(pairs):
        if t not in tables:
            tables[t] = R.table(clouds[t], p)
        want, _ = R.result(clouds[t], clouds[s], g, p, tables[t])
        assert out[e].tobytes() == want.tobytes(), (e, t, s, out[e], want)
    if n >= 3:
        tie = out[1]
        assert (tie["score"], tie["best_a"], tie["best_dx"], tie["best_dy"]) == (255, p.half_a, -2, 0)
    if n == 257:
        assert (out["status"][[3, 4, 8]] == _abi.DPG_CSM_NO_OVERLAP).all() and (out["score"][[3, 4, 8]] == 0).all()
        assert (out["best_a"][[3, 4, 8]] == p.half_a).all() and (out["best_dx"][[3, 4, 8]] == 0).all()
        assert out["status"][0] == _abi.DPG_CSM_OK


def test_batch_from_poses_equals_guesses(ctx):
    rm, clouds = _batch_store(ctx)
    p = _params(half_cells=100, half_x=5, half_y=4, half_a=3)
    est = np.array([[0, 0, 0], rm.off, [1, 1, 1], [0, 0, 0], rm.truth, [0.5, 0, 0], [0, 0, 0]], np.float32)
    edges = np.array([[0, 1], [0, 4], [4, 5]], np.int32)
    a = ctx.csm_batch(edges, poses=est, params=p)
    b = ctx.csm_batch(edges, guesses=np.stack([api.icp_guess(est[s], est[t]) for t, s in edges]), params=p)
    assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ errors
def test_errors(ctx):
    rm, clouds = _batch_store(ctx)
    p = _params(half_cells=100, half_x=5, half_y=4, half_a=3)
    edges = np.array([[0, 1], [0, 4]], np.int32)
    g = np.stack([R.guess_of(0, 0, 0)] * 2)
    est = np.zeros((len(clouds), 3), np.float32)
    with pytest.raises(_abi.DpgError, match=r"\(-1\)"):                      # the LDS budget
        ctx.csm_batch(edges, guesses=g, params=_params(half_cells=_largest_half_cells() + 1))
    with pytest.raises(_abi.DpgError, match=r"\(-1\)"):
        ctx.csm_table(0, _params(kernel_radius=8))
    with pytest.raises(_abi.DpgError, match=r"\(-1\)"):
        ctx.csm_scores(0, 1, g[0], _params(half_a=65))
    out = np.zeros(2, _abi.CSM_RESULT_DTYPE)                                 # cap too small: nothing written
    out.view(np.uint8)[:] = 7
    before = out.tobytes()
    rc = lib().dpg_csm_batch(ctx.handle, ptr(edges, C.c_int32), 2, None, ptr(g, C.c_float), C.byref(p), vptr(out), 1)
    assert rc == -4 and out.tobytes() == before
    tb = np.zeros(10, np.uint8)
    assert lib().dpg_csm_table(ctx.handle, 0, C.byref(p), ptr(tb, C.c_uint8), tb.size) == -4 and not tb.any()
    vol = np.zeros(10, np.int32)
    assert lib().dpg_csm_scores(ctx.handle, 0, 1, ptr(g[0], C.c_float), C.byref(p), ptr(vol, C.c_int32), vol.size) == -4
    for bad in ([[0, len(clouds)]], [[-1, 0]]):                              # a bad edge
        with pytest.raises(_abi.DpgError, match=r"\(-1\)"):
            ctx.csm_batch(np.array(bad, np.int32), guesses=g[:1], params=p)
    with pytest.raises(_abi.DpgError, match=r"\(-1\)"):
        ctx.csm_table(len(clouds), p)
    with pytest.raises(_abi.DpgError, match=r"\(-1\)"):                      # both, neither
        ctx.csm_batch(edges, poses=est, guesses=g, params=p)
    with pytest.raises(_abi.DpgError, match=r"\(-1\)"):
        ctx.csm_batch(edges, params=p)
    assert len(ctx.csm_batch(np.zeros((0, 2), np.int32), guesses=np.zeros((0, 6), np.float32), params=p)) == 0
    with api.Context(0) as fresh:                                            # no scans uploaded
        assert fresh.csm_kernel_ms() < 0
        with pytest.raises(_abi.DpgError, match=r"\(-3\)"):
            fresh.csm_batch(edges, guesses=g, params=p)
    with api.Context(0, virtual=2) as multi:                                 # a multi-device form
        multi.upload_scans(np.concatenate(clouds[:2]), np.array([0, 360, 720], np.int64), 1)
        for call in (lambda: multi.csm_batch(edges[:1], guesses=g[:1], params=p), lambda: multi.csm_table(0, p),
                     lambda: multi.csm_scores(0, 1, g[0], p)):
            with pytest.raises(_abi.DpgError, match=r"\(-3\)"):
                call()


# ------------------------------------------------------------------ ICP from explicit guesses
@pytest.mark.parametrize("config,n_edges", [("config1", 1), ("config2", 20)])
def test_icp_prepare_guess_equals_icp_prepare(ctx, workload, config, n_edges):
    w = workload(config)
    ip = _abi.default_icp_params()
    ctx.upload_scans(w.pts, w.offsets, ip.downsample_icp_points_ratio)
    edges = np.ascontiguousarray(w.edges[:n_edges])
    res, _ = ctx.icp_batch(edges, w.est, ip, compute_cov=False)
    guesses = np.stack([api.icp_guess(w.est[s], w.est[t]) for t, s in edges])
    res_g, _ = ctx.icp_batch_guess(edges, guesses, ip, compute_cov=False)
    assert res_g.tobytes() == res.tobytes()
    assert (res["converged"] != 0).all()
    with pytest.raises(ValueError):
        ctx.icp_prepare_guess(edges, guesses[:-1] if n_edges > 1 else np.zeros((2, 6), np.float32), ip)


# ------------------------------------------------------------------ end to end
def test_end_to_end_guess_outside_icp_basin(ctx):
    """Two scans of the room (csm_ref.Room), the source's estimate off by (-1.3 m, 1.2 m, -0.16 rad).
    The CPU oracle's ICP (downsample ratio 1, defaults otherwise), measured on the CPU:
      from the perturbed poses it ends 1.376 m and 0.100 degrees from the ground truth (> 5 cm: lost);
      from the reference-refined pose, passed as poses, 0.0015 m and 0.151 degrees (within 2.5 cm, 0.5 degrees).
    Here: csm_batch, then icp_batch_guess from its guess, must end within 5 cm and 1 degree."""
    rm = R.room()
    _upload(ctx, rm.clouds)
    ip = _abi.default_icp_params()
    ip.downsample_icp_points_ratio = 1
    edges = np.array([[0, 1]], np.int32)
    plain, _ = ctx.icp_batch(edges, rm.est, ip, compute_cov=False)
    e_plain = rm.error(plain["z"][0])
    p = _abi.default_csm_params()
    m = ctx.csm_batch(edges, poses=rm.est, params=p)
    want, _ = R.result(rm.clouds[0], rm.clouds[1], api.icp_guess(rm.est[1], rm.est[0]), p)
    assert m[0].tobytes() == want.tobytes()
    res, _ = ctx.icp_batch_guess(edges, m["guess"], ip, compute_cov=False)
    e = rm.error(res["z"][0])
    print(f"ICP from the estimates: {e_plain[0]:.4f} m {math.degrees(e_plain[1]):.3f} deg; matcher "
          f"{int(m['score'][0])} of {255 * int(m['n_src'][0])} (at the guess {int(m['score_at_guess'][0])}); "
          f"ICP from its guess: {e[0]:.4f} m {math.degrees(e[1]):.3f} deg; kernel {ctx.csm_kernel_ms():.3f} ms")
    assert e_plain[0] > 0.05 or e_plain[1] > math.radians(1.0)       # what the matcher is for
    assert res["converged"][0] and e[0] <= 0.05 and e[1] <= math.radians(1.0)


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


def test_slam_prematch_option():
    from dpgslam import synth
    from dpgslam.slam import DpgSLAM, GpuBackend

    class Recording(GpuBackend):
        def prematch(self, clouds, edges, est, cp, ratio):
            self.rec_pre = (np.array(edges), np.array(est))
            return super().prematch(clouds, edges, est, cp, ratio)

        def icp_batch_guess(self, clouds, edges, guesses, n_nodes, p):
            r = super().icp_batch_guess(clouds, edges, guesses, n_nodes, p)
            self.rec_icp = (np.array(edges), np.array(guesses), r.copy())
            return r

    w = synth.make_dynamic(n_passes=2, nodes_per_pass=8, n_beams=360, world_size=16.0, range_max=8.0, n_boxes=6, seed=9)
    cp = _abi.default_csm_params()
    runs = {}
    for name, kw in (("off", {}), ("never", dict(loop_closure_prematch=cp, prematch_min_response=1.5)),
                     ("always", dict(loop_closure_prematch=cp, prematch_min_response=0.0))):
        with api.Context(0) as c:
            be = Recording(c)
            s = DpgSLAM(backend=be, **kw)
            _drive_two_passes(s, w)
            runs[name] = (s.factors.tobytes(), s.poses.tobytes(), s.n_factors)
            if name == "always":   # the sweep's alignments: the matcher and the ICP called by hand on the same candidates
                lc, est = be.rec_pre
                edges, guesses, res = be.rec_icp
                n_succ = len(edges) - len(lc)
                assert len(lc) > 0 and np.array_equal(edges[n_succ:], lc)
                m = c.csm_batch(lc, poses=est, params=cp)
                assert m.tobytes() == s.last_prematch.tobytes()
                g = np.stack([api.icp_guess(est[b], est[a]) for a, b in edges])
                g[n_succ:] = m["guess"]
                assert g.tobytes() == guesses.tobytes()
                by_hand, _ = c.icp_batch_guess(edges, g, s.icp_params, compute_cov=False)
                assert by_hand.tobytes() == res.tobytes()
            elif name == "never":
                assert s.last_prematch is not None and len(s.last_prematch) > 0
    assert runs["never"] == runs["off"]
