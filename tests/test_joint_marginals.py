"""Joint marginals and relative-pose covariances of ANY node pair (gtsam::Marginals::
jointMarginalCovariance) from root paths of the Cholesky factor on the GPU (dpg_chol_sel.hip
chol_path_forward / chol_path_dot), against H^-1 on the CPU.

Reference and tolerance are those of tests/test_marginals.py: per graph tol = max(1e-12, 100 x d),
d the largest block-wise disagreement of np.linalg.inv against cho_solve over the diagonal blocks
AND the queried off-diagonal blocks (dense_reference's pairs=); a graph whose rule gives more than
1e-6 is rejected.  Relative covariances: the same rule on the 3x3 results J S J^T of the two CPU
routes, J from oracle.linearize of an exactly consistent Between factor.  The references have keys
of their own ("... joint"), so the tolerances of tests/test_marginals.py are what they were.
"""
import ctypes as C

import numpy as np
import pytest

from graphs import consistent_mesh_graph, gtsam_test_graph
from test_marginals import (BETWEEN, band_graph, blk, chain_graph, dense_h, dense_reference, err_code, graph_from_pairs,
                            mesh900, rel_err, rel_pose, solver_options)

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3


# ------------------------------------------------------------------------------------ CPU reference
def random_pairs(V, n, seed, extra=()):
    rng = np.random.default_rng(seed)
    pr = [(int(a), int(b)) for a, b in rng.integers(0, V, (n, 2))]
    return pr + [(int(a), int(b)) for a, b in extra]


def check_pairs(name, got, S, tol, pairs):
    errs = [rel_err(got[q], blk(S, i, j)) for q, (i, j) in enumerate(pairs)]
    print(f"[{name}] {len(pairs)} blocks, max block error {max(errs):.3g} (tol {tol:.3g})")
    assert max(errs) <= tol, (name, max(errs), tol, pairs[int(np.argmax(errs))])


def jacobian(X, i, j):
    """J = [A_i A_j] of the Between linearization at zero error (oracle.linearize)."""
    from oracle import oracle as O
    from dpgslam import api
    e, Ai, Aj = O.linearize(api.between_factor(i, j, rel_pose(X, i, j), (0.1, 0.1, 0.05)), X)
    assert np.abs(e).max() < 1e-12
    return np.hstack([Ai, Aj])


_REL = {}


def relative_reference(key, F, X, pairs):
    """([J S J^T per pair], tol): S from np.linalg.inv; the tolerance rule on the 3x3 results of
    the two CPU routes (inv, cho_solve).  Computed once per key."""
    if key not in _REL:
        import scipy.linalg as sl
        H = dense_h(F, X)
        S1 = np.linalg.inv(H)
        S2 = sl.cho_solve(sl.cho_factor(H), np.eye(len(H)))
        ref, d = [], 0.0
        for i, j in pairs:
            if i == j:
                ref.append(np.zeros((3, 3)))
                continue
            J = jacobian(X, i, j)
            r = []
            for S in (S1, S2):
                Sb = np.block([[blk(S, i, i), blk(S, i, j)], [blk(S, j, i), blk(S, j, j)]])
                r.append(J @ Sb @ J.T)
            ref.append(r[0])
            d = max(d, rel_err(r[1], r[0]))
        tol = max(1e-12, 100.0 * d)
        print(f"[{key}] relative covariances: CPU disagreement = {d:.2g}  tol = {tol:.2g}")
        assert tol <= 1e-6, f"{key}: not a valid input for the tolerance rule ({tol:.2g})"
        _REL[key] = (ref, tol)
    return _REL[key]


def check_relative(name, got, ref, tol, pairs):
    errs = []
    for q, (i, j) in enumerate(pairs):
        assert np.array_equal(got[q], got[q].T), (name, i, j)
        if i == j:
            assert np.all(got[q] == 0.0), (name, i)
        else:
            errs.append(rel_err(got[q], ref[q]))
    print(f"[{name}] relative covariances: max error {max(errs):.3g} (tol {tol:.3g})")
    assert max(errs) <= tol, (name, max(errs), tol)


# -------------------------------------------------------------------------------------------- tests
def test_smallest_graphs(ctx):
    """One node with a prior: pair (0, 0), a single root front.  Two nodes: all four pairs; the
    relative covariance of (0, 1) is the Between factor's own covariance."""
    from dpgslam import api
    F1 = api.prior_factor(0, (1.0, -2.0, 0.3), (0.2, 0.3, 0.1))
    X1 = np.array([[1.1, -2.0, 0.25]])
    S, tol = dense_reference("one node joint", F1, X1, pairs=[(0, 0)])
    ctx.gn_setup(1, F1)
    ctx.gn_set_poses(X1)
    check_pairs("one node", ctx.gn_cross_covariances([(0, 0)]), S, tol, [(0, 0)])
    assert np.all(ctx.gn_relative_covariances([(0, 0)]) == 0.0)
    J1 = ctx.gn_joint_marginal([0])
    assert J1.shape == (3, 3) and rel_err(J1, S) <= tol
    X2 = np.array([[0.0, 0.1, 0.2], [1.0, 0.3, -0.4]])
    F2 = np.concatenate([api.prior_factor(0, (0.0, 0.0, 0.0), (0.2, 0.2, 0.1)),
                         api.between_factor(0, 1, (1.0, 0.0, -0.5), (0.1, 0.1, 0.05))])
    pairs = [(0, 1), (1, 0), (0, 0), (1, 1)]
    S, tol = dense_reference("two nodes joint", F2, X2, pairs=pairs)
    ctx.gn_setup(2, F2)
    ctx.gn_set_poses(X2)
    P = ctx.gn_cross_covariances(pairs)
    check_pairs("two nodes", P, S, tol, pairs)
    assert np.array_equal(P[1], P[0].T)
    R = ctx.gn_relative_covariances([(0, 1)])[0]
    print(f"[two nodes] relative covariance error {np.abs(R - np.diag([0.01, 0.01, 0.0025])).max():.3g}")
    assert np.abs(R - np.diag([0.01, 0.01, 0.0025])).max() <= 1e-12, R


def test_gtsam_test_all_pairs_and_joint(ctx):
    _, F, X = gtsam_test_graph()
    pairs = [(i, j) for i in range(5) for j in range(5)]
    S, tol = dense_reference("gtsam_test joint", F, X, pairs=pairs)
    ctx.gn_setup(5, F)
    ctx.gn_set_poses(X)
    P = ctx.gn_cross_covariances(pairs)
    check_pairs("gtsam_test", P, S, tol, pairs)
    for i in range(5):
        for j in range(5):
            assert np.array_equal(P[5 * j + i], P[5 * i + j].T)
    Jm = ctx.gn_joint_marginal([0, 1, 2, 3, 4])
    assert Jm.shape == (15, 15) and np.array_equal(Jm, Jm.T)
    check_pairs("gtsam_test joint", [blk(Jm, i, j) for i, j in pairs], S, tol, pairs)
    assert np.linalg.eigvalsh(Jm).min() > 0.0
    sub = ctx.gn_joint_marginal([3, 1])
    want = np.block([[blk(Jm, 3, 3), blk(Jm, 3, 1)], [blk(Jm, 1, 3), blk(Jm, 1, 1)]])
    assert sub.tobytes() == want.tobytes()


def test_disconnected_components(ctx):
    """Two 6-node chains, each with its own prior: a forest.  Cross blocks are exactly 0.0."""
    from dpgslam import api
    X, _ = chain_graph(V=12, seed=21)
    sig = (0.1, 0.1, 0.05)
    F = np.concatenate([graph_from_pairs(X, [(i, i + 1) for i in range(5)] + [(i, i + 1) for i in range(6, 11)], sig),
                        api.prior_factor(6, tuple(X[6]), sig)])
    inside = [(i, j) for i in range(6) for j in range(6)] + [(i, j) for i in range(6, 12) for j in range(6, 12)]
    across = [(0, 6), (6, 0), (5, 11), (3, 8), (11, 2)]
    S, tol = dense_reference("two chains joint", F, X, pairs=inside)
    for order in ("md", "nd"):
        with solver_options(ctx, order=order):
            ctx.gn_setup(12, F)
            ctx.gn_set_poses(X)
            check_pairs(f"two chains {order}", ctx.gn_cross_covariances(inside), S, tol, inside)
            Z = ctx.gn_cross_covariances(across)
            Jm = ctx.gn_joint_marginal(list(range(12)))
        assert np.all(Z == 0.0) and not np.any(np.signbit(Z))
        assert np.all(Jm[:18, 18:] == 0.0) and np.all(Jm[18:, :18] == 0.0) and np.array_equal(Jm, Jm.T)


def chain_pairs(V):
    # adjacent nodes are an ancestor / descendant pair or two columns of one supernode (both occur
    # along a stretch of a chain), the rest are far apart: deep paths
    extra = [(0, V - 1), (V - 1, 0), (77, 77), (10, 11), (11, 12), (12, 13), (13, 14), (14, 10), (V - 2, V - 1)]
    return random_pairs(V, 40, 101, extra)


@pytest.mark.parametrize("opts", [{"order": "md"}, {"order": "nd"}, {"max_supernode_cols": 2, "relax_fraction": 0.0}],
                         ids=["md", "nd", "tiny-fronts"])
def test_chain_thin_and_deep(ctx, opts):
    X, F = chain_graph()
    V = len(X)
    pairs = chain_pairs(V)
    S, tol = dense_reference("chain200 joint", F, X, pairs=pairs)
    ref, rtol = relative_reference("chain200 joint", F, X, pairs)
    with solver_options(ctx, **opts):
        ctx.gn_setup(V, F)
        ctx.gn_set_poses(X)
        P = ctx.gn_cross_covariances(pairs)
        R = ctx.gn_relative_covariances(pairs)
    check_pairs(f"chain200 {opts}", P, S, tol, pairs)
    assert np.array_equal(P[41], P[40].T)
    check_relative(f"chain200 {opts}", R, ref, rtol, pairs)


@pytest.mark.parametrize("order", ["auto", "md"])
def test_band_graph_large_fronts(ctx, order):
    """130 nodes, band 70.  Under the default order a front has all 130 block rows: the path
    solve's vectors are past their LDS bound and live in the global work buffer; under minimum
    degree the largest front (113) is the largest that still works in LDS."""
    X, F = band_graph()
    V = len(X)
    pairs = random_pairs(V, 40, 7, [(0, V - 1), (V - 1, 0), (64, 64)])
    S, tol = dense_reference("band130 joint", F, X, pairs=pairs)
    with solver_options(ctx, order=order):
        ctx.gn_setup(V, F)
        ctx.gn_set_poses(X)
        P = ctx.gn_cross_covariances(pairs)
    check_pairs(f"band130 {order}", P, S, tol, pairs)


def mesh_pairs():
    X0, _, shared = mesh900()
    V = len(X0)
    return random_pairs(V, 60, 17, [(0, V - 1), (V - 1, 0), (450, 450)]), shared, [(i, i) for i in range(0, V, 37)]


@pytest.mark.parametrize("fused", [1, 0], ids=["dag", "levels"])
def test_mesh_random_pairs_and_cross_checks(ctx, fused):
    """consistent_mesh_graph(V=900) at the perturbed poses, the factor from the one-launch DAG path
    and from the level path.  Two independent device routes agree: (i, i) against the selected
    inverse's diagonal blocks, pairs that share a factor against gn_marginal_pairs."""
    X0, F, _ = mesh900()
    V = len(X0)
    pairs, shared, diag = mesh_pairs()
    S, tol = dense_reference("mesh900 joint", F, X0, pairs=pairs + shared)
    ref, rtol = relative_reference("mesh900 joint", F, X0, pairs)
    with solver_options(ctx, fused=fused):
        ctx.gn_setup(V, F)
        ctx.gn_set_poses(X0)
        P = ctx.gn_cross_covariances(pairs)
        R = ctx.gn_relative_covariances(pairs)
        D = ctx.gn_cross_covariances(diag)
        M = ctx.gn_marginals([i for i, _ in diag])
        Q = ctx.gn_cross_covariances(shared)
        Q2 = ctx.gn_marginal_pairs(shared)
    check_pairs(f"mesh900 fused={fused}", P, S, tol, pairs)
    check_relative(f"mesh900 fused={fused}", R, ref, rtol, pairs)
    check_pairs(f"mesh900 fused={fused} diagonal", D, S, tol, diag)
    e1 = max(rel_err(D[q], M[q]) for q in range(len(diag)))
    e2 = max(rel_err(Q[q], Q2[q]) for q in range(len(shared)))
    print(f"[mesh900 fused={fused}] path route against selected inverse: diagonal {e1:.3g}, factor pairs {e2:.3g} (tol {tol:.3g})")
    assert e1 <= tol and e2 <= tol


def test_deterministic_and_leaves_everything_alone(ctx):
    """Two calls are bitwise equal; the Gauss-Newton loop and the selected inverse give bitwise the
    same with a joint call in between; L11^-1 kept beside the fronts (solve_inv_cols) changes nothing."""
    X0, F, _ = mesh900()
    V = len(X0)
    pairs, _, _ = mesh_pairs()
    nodes = [5, 800, 33, 5, 412]
    ctx.gn_setup(V, F)
    ctx.gn_set_poses(X0)
    m0 = ctx.gn_marginals()
    a = ctx.gn_cross_covariances(pairs)
    b = ctx.gn_cross_covariances(pairs)
    assert a.tobytes() == b.tobytes()
    ja, jb = ctx.gn_joint_marginal(nodes), ctx.gn_joint_marginal(nodes)
    assert ja.tobytes() == jb.tobytes() and np.array_equal(ja, ja.T)
    assert ctx.gn_relative_covariances(pairs).tobytes() == ctx.gn_relative_covariances(pairs).tobytes()
    assert ctx.gn_marginals().tobytes() == m0.tobytes()
    ctx.gn_set_poses(X0)
    s0, Xa = ctx.gn_run(V)
    n0 = ctx.gn_factorizations()
    ctx.gn_set_poses(X0)
    c = ctx.gn_cross_covariances(pairs)
    assert c.tobytes() == a.tobytes()
    ctx.gn_joint_marginal(nodes), ctx.gn_relative_covariances(pairs[:5])
    s1, Xb = ctx.gn_run(V)
    assert Xa.tobytes() == Xb.tobytes()
    assert s1["iterations"] == s0["iterations"] and ctx.gn_factorizations() == n0
    assert s1["final_error"] == s0["final_error"]
    with solver_options(ctx, solve_inv_cols=12):
        ctx.gn_setup(V, F)
        ctx.gn_set_poses(X0)
        d = ctx.gn_cross_covariances(pairs)
    assert d.tobytes() == a.tobytes()


def test_errors_write_nothing(ctx):
    """DPG_ERR_ARG / DPG_ERR_STATE cases through raw ctypes; the output keeps its sentinel."""
    from dpgslam import _abi, api
    from dpgslam._abi import lib, ptr
    X, F = chain_graph(V=12)
    V = len(X)
    sent = 12345.678
    L = lib()
    pair_fns = ["cross_covariances", "relative_covariances"]

    def raw(fn, handle, idx, n=None, null=False):
        a = np.ascontiguousarray(idx, np.int32)
        out = np.full(9 * max(a.size, 1) ** 2, sent)
        k = (len(a) if n is None else n)
        rc = fn(handle, None if null else ptr(a, C.c_int32), k, ptr(out, C.c_double))
        assert np.all(out == sent), fn
        return rc

    def all_fail(prefix, handle, code):
        for name in pair_fns:
            assert raw(getattr(L, f"{prefix}_{name}"), handle, [(0, 1)]) == code, name
        assert raw(getattr(L, f"{prefix}_joint_marginal"), handle, [0, 1]) == code

    ctx.gn_setup(V, F)
    ctx.gn_set_poses(X)
    for name in pair_fns:
        fn = getattr(L, f"dpg_gn_{name}")
        assert raw(fn, ctx.handle, [(0, 1), (3, V)]) == ARG
        assert raw(fn, ctx.handle, [(-1, 2)]) == ARG
        assert raw(fn, ctx.handle, [(0, 1)], null=True) == ARG
        assert raw(fn, ctx.handle, [(0, 1)], n=-1) == ARG
    fn = L.dpg_gn_joint_marginal
    assert raw(fn, ctx.handle, [0, V]) == ARG
    assert raw(fn, ctx.handle, [3, -1]) == ARG
    assert raw(fn, ctx.handle, [0, 1], null=True) == ARG
    with pytest.raises(_abi.DpgError) as e:
        ctx.gn_cross_covariances([(0, V)])
    assert err_code(e) == ARG
    # the pattern-restricted call still refuses what it refused
    with pytest.raises(_abi.DpgError) as e:
        ctx.gn_marginal_pairs([(4, 6)])
    assert err_code(e) == ARG
    assert np.all(np.isfinite(ctx.gn_cross_covariances([(4, 6), (0, V - 1)])))
    # no Cholesky: the graph was set up for PCG
    gp = _abi.default_gn_params()
    gp.linear_solver = _abi.DPG_SOLVER_PCG
    ctx.gn_setup(V, F, params=gp)
    ctx.gn_set_poses(X)
    all_fail("dpg_gn", ctx.handle, STATE)
    ctx.gn_setup(V, F)
    with api.Context(0) as fresh:   # before any setup
        all_fail("dpg_gn", fresh.handle, STATE)
    with api.Context(0, virtual=2) as two:   # more than one rank
        two.gn_setup(V, F)
        two.gn_set_poses(X)
        all_fail("dpg_gn", two.handle, STATE)
    g = api.IncGraph(ctx, mode="isam2")   # before its first update
    try:
        all_fail("dpg_inc", g.handle, STATE)
        last = np.maximum(F["i"], np.where(F["kind"] == BETWEEN, F["j"], 0))
        for v in range(3):
            g.update(X[v:v + 1], F[last == v])
        for name in pair_fns:
            fn = getattr(L, f"dpg_inc_{name}")
            assert raw(fn, g.handle, [(0, 3)]) == ARG
            assert raw(fn, g.handle, [(0, 1)], null=True) == ARG
        assert raw(L.dpg_inc_joint_marginal, g.handle, [0, -1]) == ARG
        assert np.all(np.isfinite(g.cross_covariances([(0, 2)])))
    finally:
        g.close()


def inc_pairs(k):
    return random_pairs(k, 12, 1000 + k, [(0, k - 1), (k - 1, 0), (2, 2)])


def _inc_joint_sequence(ctx, X0, F, with_joint, full_refactor=False, checks=()):
    """One node per update (tests/test_marginals.py's sequence); the joint results and the exported
    state after the updates in `checks`."""
    from dpgslam import api
    g = api.IncGraph(ctx, mode="isam2", reorder_every=8, full_refactor=full_refactor)
    last = np.maximum(F["i"], np.where(F["kind"] == BETWEEN, F["j"], 0))
    est, got = [], {}
    try:
        for v in range(len(X0)):
            g.update(X0[v:v + 1], F[last == v])
            if with_joint and (v + 1) in checks:
                pr = inc_pairs(v + 1)
                got[v + 1] = (g.cross_covariances(pr), g.relative_covariances(pr), g.joint_marginal([0, v, v // 2]),
                              g.export_state())
            est.append(g.poses().copy())
    finally:
        g.close()
    return est, got


def test_incremental_graph(ctx):
    """ISAM2-mode updates with reorders and moved fronts: the blocks match H^-1 at theta, are
    bitwise those of full refactorizations, and leave the estimates bitwise alone."""
    X0, F, _ = consistent_mesh_graph(V=64, k=6)
    keep = (F["i"] < 60) & ((F["kind"] != BETWEEN) | (F["j"] < 60))
    X0, F = X0[:60], F[keep]
    checks = (5, 17, 33, 60)
    est_a, got_a = _inc_joint_sequence(ctx, X0, F, True, checks=checks)
    assert sorted(got_a) == list(checks)
    for k in checks:
        P, R, Jm, stt = got_a[k]
        pr = inc_pairs(k)
        S, tol = dense_reference(f"inc60@{k} joint", stt["factors"], stt["theta"], pairs=pr)
        ref, rtol = relative_reference(f"inc60@{k} joint", stt["factors"], stt["theta"], pr)
        check_pairs(f"inc60@{k}", P, S, tol, pr)
        check_relative(f"inc60@{k}", R, ref, rtol, pr)
        assert np.array_equal(Jm, Jm.T) and rel_err(blk(Jm, 0, 1), blk(S, 0, k - 1)) <= tol
    _, got_b = _inc_joint_sequence(ctx, X0, F, True, full_refactor=True, checks=checks)
    for k in checks:
        for q in range(3):
            assert got_a[k][q].tobytes() == got_b[k][q].tobytes(), (k, q)
    est_c, _ = _inc_joint_sequence(ctx, X0, F, False)
    for a, c in zip(est_a, est_c):
        assert a.tobytes() == c.tobytes()


def test_slam_get_relative_pose_covariance():
    """DpgSLAM.GetRelativePoseCovariance over the short synthetic session of
    test_slam_get_pose_covariance."""
    from dpgslam import api, synth
    from dpgslam.slam import DpgSLAM
    w = synth.make_dynamic(n_passes=2, nodes_per_pass=14, n_beams=360, world_size=16.0, range_max=8.0, n_boxes=6,
                           seed=9)
    rng = np.random.default_rng(3)
    with api.Context(0) as c:
        s = DpgSLAM(backend="gpu", ctx=c)
        for p in range(len(w.pass_start) - 1):
            if p:
                s.incrementPassNumber()
            for v in range(int(w.pass_start[p]), int(w.pass_start[p + 1])):
                odom = w.est[v].astype(np.float64) + rng.normal(0, [0.01, 0.01, 0.002])
                s.ObserveOdometry(odom[:2].astype(np.float32), np.float32(odom[2]))
                s.ObserveLaser(w.ranges[v], 0.0, float(w.geom[v, 2]), float(w.geom[v, 0]), float(w.geom[v, 1]))
        V = len(s.poses)
        assert V > 10
        for i, j in ((0, V - 1), (V - 1, 3), (2, 9)):
            cov = s.GetRelativePoseCovariance(i, j)
            assert cov.shape == (3, 3) and np.array_equal(cov, cov.T)
            assert np.linalg.eigvalsh(cov).min() > 0.0
            assert np.array_equal(cov, s.be.inc.relative_covariances([(i, j)])[0])
        assert np.all(s.GetRelativePoseCovariance(4, 4) == 0.0)
        with pytest.raises(IndexError):
            s.GetRelativePoseCovariance(0, V)
        with pytest.raises(IndexError):
            s.GetRelativePoseCovariance(V, 0)
