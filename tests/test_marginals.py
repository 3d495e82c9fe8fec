"""Marginal pose covariances (gtsam::Marginals / ISAM2::marginalCovariance) by selected inversion
of the Cholesky factor on the GPU (dpg_chol_sel.hip chol_selinv_level), against H^-1 on the CPU.

Reference: H = sum A^T Omega A from oracle.linearize, dense (sparse for config 3).  Every 3x3 block
is compared by |S_gpu - S_ref|_F / |S_ref|_F.  The tolerance is not fixed: per graph it is
max(1e-12, 100 x d), d the largest block-wise disagreement of two fp64 CPU routes with different
elimination -- np.linalg.inv against cho_solve(cho_factor(H), I); splu NATURAL against COLAMD for
the sparse case.  (100: the GPU's nested-dissection order is a third elimination order.)  A graph
whose rule gives more than 1e-6 is rejected as an input.

d of each graph as measured on the CPU (it varies a little with the BLAS; the tests print theirs):
  gtsam_test at its optimum                 5e-15   (cond 7e2)
  one node / two nodes                      < 1e-15
  200-node chain                            5e-10 .. 9e-10   (cond 6e8)
  consistent_mesh_graph(V=900) at X0        2e-11 .. 4e-11   (cond 3e7)
  130-node band graph                       1e-11 .. 2e-11   (cond 9e7)
  config 3 after optimize_graph (sparse)    1.6e-10
  consistent_mesh_graph(V=64)[:60] at theta 2e-15, 1e-13, 2e-14, 2e-13 after updates 5, 17, 33, 60
"""
import math
import re

import numpy as np
import pytest

from graphs import consistent_mesh_graph, gtsam_test_graph

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3
BETWEEN = 1   # DPG_FACTOR_BETWEEN


# ------------------------------------------------------------------------------------ CPU reference
def h_blocks(F, X):
    """The 3x3 blocks of H = sum A^T Omega A at X: (rows, cols, values), duplicates to be summed."""
    from oracle import oracle as O
    from dpgslam import _abi
    X = np.asarray(X, np.float64)
    ri, ci, vv = [], [], []
    for f in F:
        _, Ai, Aj = O.linearize(f, X)
        W = np.diag(np.asarray(f["info"], np.float64))
        i, j = int(f["i"]), int(f["j"])
        ri.append(i), ci.append(i), vv.append(Ai.T @ W @ Ai)
        if int(f["kind"]) == _abi.DPG_FACTOR_BETWEEN:
            ri.append(j), ci.append(j), vv.append(Aj.T @ W @ Aj)
            ri.append(i), ci.append(j), vv.append(Ai.T @ W @ Aj)
            ri.append(j), ci.append(i), vv.append(Aj.T @ W @ Ai)
    return np.array(ri), np.array(ci), np.array(vv)


def dense_h(F, X):
    V = len(X)
    H = np.zeros((V, 3, V, 3))
    r, c, v = h_blocks(F, X)
    np.add.at(H, (r, slice(None), c), v)   # H[r, a, c, b] += v[a, b]
    return H.reshape(3 * V, 3 * V)


def sparse_h(F, X):
    import scipy.sparse as sp
    V = len(X)
    r, c, v = h_blocks(F, X)
    a, b = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
    rows = (3 * r[:, None, None] + a[None]).ravel()
    cols = (3 * c[:, None, None] + b[None]).ravel()
    return sp.csc_matrix((v.ravel(), (rows, cols)), shape=(3 * V, 3 * V))


def blk(S, i, j):
    return S[3 * i:3 * i + 3, 3 * j:3 * j + 3]


def rel_err(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


_REF = {}


def dense_reference(key, F, X, pairs=()):
    """(Sigma, tol) of a graph, computed once per key: the dense inverse and the tolerance rule."""
    if key not in _REF:
        import scipy.linalg as sl
        H = dense_h(F, X)
        S1 = np.linalg.inv(H)
        S2 = sl.cho_solve(sl.cho_factor(H), np.eye(len(H)))
        V = len(X)
        d = max(rel_err(blk(S2, i, i), blk(S1, i, i)) for i in range(V))
        for i, j in pairs:
            d = max(d, rel_err(blk(S2, i, j), blk(S1, i, j)))
        tol = max(1e-12, 100.0 * d)
        print(f"[{key}] cond(H) = {np.linalg.cond(H):.2g}  CPU disagreement = {d:.2g}  tol = {tol:.2g}")
        assert tol <= 1e-6, f"{key}: not a valid input for the tolerance rule ({tol:.2g})"
        S1.setflags(write=False)
        _REF[key] = (S1, tol)
    return _REF[key]


def check_nodes(name, got, S, tol, nodes=None):
    nodes = range(len(got)) if nodes is None else nodes
    errs = [rel_err(got[q], blk(S, i, i)) for q, i in enumerate(nodes)]
    print(f"[{name}] max block error {max(errs):.3g} (tol {tol:.3g})")
    assert max(errs) <= tol, (name, max(errs), tol, int(np.argmax(errs)))


# ------------------------------------------------------------------------------------------- graphs
def rel_pose(X, i, j):
    c, s = math.cos(X[i, 2]), math.sin(X[i, 2])
    dx, dy = X[j, 0] - X[i, 0], X[j, 1] - X[i, 1]
    d = X[j, 2] - X[i, 2]
    return (c * dx + s * dy, -s * dx + c * dy, math.atan2(math.sin(d), math.cos(d)))


def graph_from_pairs(X, pairs, sig=(0.1, 0.1, 0.05)):
    """Exactly consistent Between factors over `pairs` at the poses X, one prior on node 0."""
    from dpgslam import api
    F = [api.prior_factor(0, tuple(X[0]), sig)]
    F += [api.between_factor(i, j, rel_pose(X, i, j), sig) for i, j in pairs]
    return np.concatenate(F)


def chain_graph(V=200, seed=5):
    rng = np.random.default_rng(seed)
    X = np.column_stack([np.cumsum(rng.uniform(0.5, 1.5, V)), rng.normal(0, 0.5, V), rng.uniform(-math.pi, math.pi, V)])
    return X, graph_from_pairs(X, [(i, i + 1) for i in range(V - 1)])


def band_graph(V=130, band=70, seed=7):
    rng = np.random.default_rng(seed)
    X = np.column_stack([rng.uniform(0, 20, V), rng.uniform(0, 20, V), rng.uniform(-math.pi, math.pi, V)])
    return X, graph_from_pairs(X, [(i, j) for i in range(V) for j in range(i + 1, min(V, i + band + 1))])


_MESH = {}


def mesh900():
    if "m" not in _MESH:
        X0, F, _ = consistent_mesh_graph(V=900, k=6)
        b = F[F["kind"] == BETWEEN]
        rng = np.random.default_rng(3)
        pick = rng.choice(len(b), 25, replace=False)
        pairs = [(int(b["i"][q]), int(b["j"][q])) for q in pick]
        pairs = pairs + [(j, i) for i, j in pairs]
        _MESH["m"] = (X0, F, pairs)
    return _MESH["m"]


class solver_options:
    """dpg_ctx_set_solver_options for the graphs set up inside, the defaults restored afterwards."""

    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        self.ctx.set_solver_options(**self.kw)

    def __exit__(self, *a):
        self.ctx.set_solver_options()


def err_code(excinfo):
    return int(re.search(r"failed \((-?\d+)\)", str(excinfo.value)).group(1))


# -------------------------------------------------------------------------------------------- tests
def test_known_answer_gtsam_test(ctx):
    """gtsam_test at its optimum: node 0 carries the only prior and every other factor is relative,
    so its marginal is the prior's covariance; both entry points give the same five blocks."""
    _, F, X_opt = gtsam_test_graph()
    S, tol = dense_reference("gtsam_test", F, X_opt)
    a = ctx.marginals(X_opt, F)
    ctx.gn_setup(len(X_opt), F)
    ctx.gn_set_poses(X_opt)
    b = ctx.gn_marginals()
    assert a.shape == (5, 3, 3) and np.array_equal(a, b)
    assert np.abs(a[0] - np.diag([0.09, 0.09, 0.01])).max() <= 1e-12, a[0]
    check_nodes("gtsam_test", a, S, tol)
    sub = ctx.gn_marginals([4, 0, 2])
    assert np.array_equal(sub, a[[4, 0, 2]])


def test_smallest_graphs(ctx):
    """One node with one prior (a root front and nothing else); two nodes, a prior and a Between."""
    from dpgslam import api
    F1 = api.prior_factor(0, (1.0, -2.0, 0.3), (0.2, 0.3, 0.1))
    X1 = np.array([[1.1, -2.0, 0.25]])
    S, tol = dense_reference("one node", F1, X1)
    check_nodes("one node", ctx.marginals(X1, F1), S, tol)
    X2 = np.array([[0.0, 0.1, 0.2], [1.0, 0.3, -0.4]])
    F2 = np.concatenate([api.prior_factor(0, (0.0, 0.0, 0.0), (0.2, 0.2, 0.1)),
                         api.between_factor(0, 1, (1.0, 0.0, -0.5), (0.1, 0.1, 0.05))])
    S, tol = dense_reference("two nodes", F2, X2, pairs=[(0, 1), (1, 0)])
    check_nodes("two nodes", ctx.marginals(X2, F2), S, tol)
    ctx.gn_setup(2, F2)
    ctx.gn_set_poses(X2)
    P = ctx.gn_marginal_pairs([(0, 1), (1, 0)])
    assert rel_err(P[0], blk(S, 0, 1)) <= tol and np.array_equal(P[1], P[0].T)


@pytest.mark.parametrize("opts", [{"order": "md"}, {"order": "nd"}, {"max_supernode_cols": 2, "relax_fraction": 0.0}],
                         ids=["md", "nd", "tiny-fronts"])
def test_chain_thin_and_deep(ctx, opts):
    """A 200-node chain: a long parent chain and a gather at every level (with two-column supernodes
    and no relaxation: many tiny fronts)."""
    X, F = chain_graph()
    S, tol = dense_reference("chain200", F, X)
    with solver_options(ctx, **opts):
        got = ctx.marginals(X, F)
    check_nodes(f"chain200 {opts}", got, S, tol)


@pytest.mark.parametrize("fused", [1, 0], ids=["dag", "levels"])
def test_mesh_all_nodes_and_pairs(ctx, fused):
    """consistent_mesh_graph(V=900) at the perturbed poses (the errors enter the Jacobians), the
    factor from the one-launch DAG path and from the level path; 50 joint blocks of factor pairs in
    both orientations."""
    X0, F, pairs = mesh900()
    S, tol = dense_reference("mesh900", F, X0, pairs=pairs)
    with solver_options(ctx, fused=fused):
        ctx.gn_setup(len(X0), F)
        ctx.gn_set_poses(X0)
        got = ctx.gn_marginals()
        P = ctx.gn_marginal_pairs(pairs)
    check_nodes(f"mesh900 fused={fused}", got, S, tol)
    errs = [rel_err(P[q], blk(S, i, j)) for q, (i, j) in enumerate(pairs)]
    print(f"[mesh900 pairs] max block error {max(errs):.3g}")
    assert max(errs) <= tol
    h = len(pairs) // 2
    for q in range(h):
        assert np.array_equal(P[h + q], P[q].T)


def test_band_graph_large_fronts(ctx):
    """130 nodes, Between factors (i, j) for 0 < j - i <= 70: fronts past any LDS bound and
    supernodes at the 64-column cap (the global-memory path)."""
    X, F = band_graph()
    S, tol = dense_reference("band130", F, X)
    check_nodes("band130", ctx.marginals(X, F), S, tol)


def test_config3_against_sparse_solves(ctx, workload):
    """Config 3 (V = 2000, ICP factors, poses after optimize_graph): 20 nodes over the order against
    sparse solves with three unit columns each."""
    from scipy.sparse.linalg import splu
    from dpgslam import _abi
    w = workload("config3")
    p = _abi.default_icp_params()
    ctx.upload_scans(w.pts, w.offsets, 5)
    res, _ = ctx.icp_batch(w.edges, w.est, p, compute_cov=False)
    F = w.factors_with_icp(res, p)
    X, _ = ctx.optimize_graph(w.est.astype(np.float64), F)
    V = len(X)
    nodes = sorted(set(np.linspace(0, V - 1, 20).astype(int).tolist()))
    assert nodes[0] == 0 and nodes[-1] == V - 1 and len(nodes) == 20
    H = sparse_h(F, X)
    E = np.zeros((3 * V, 3 * len(nodes)))
    for q, i in enumerate(nodes):
        E[3 * i:3 * i + 3, 3 * q:3 * q + 3] = np.eye(3)
    A = splu(H, permc_spec="NATURAL").solve(E)
    B = splu(H, permc_spec="COLAMD").solve(E)
    ref = [A[3 * i:3 * i + 3, 3 * q:3 * q + 3] for q, i in enumerate(nodes)]
    d = max(rel_err(B[3 * i:3 * i + 3, 3 * q:3 * q + 3], ref[q]) for q, i in enumerate(nodes))
    tol = max(1e-12, 100.0 * d)
    print(f"[config3] CPU disagreement (splu NATURAL / COLAMD) = {d:.2g}  tol = {tol:.2g}")
    assert tol <= 1e-6
    got = ctx.marginals(X, F, nodes)
    errs = [rel_err(got[q], ref[q]) for q in range(len(nodes))]
    print(f"[config3] max block error {max(errs):.3g}")
    assert max(errs) <= tol, (max(errs), tol)


def test_deterministic_and_leaves_the_loop_alone(ctx):
    """Two calls are bitwise equal; set_poses(X0) + gn_run gives bitwise the same poses, iterations
    and factorization count with a marginals call in between."""
    X0, F, _ = mesh900()
    V = len(X0)
    ctx.gn_setup(V, F)
    ctx.gn_set_poses(X0)
    a = ctx.gn_marginals()
    b = ctx.gn_marginals()
    assert a.tobytes() == b.tobytes()
    ctx.gn_set_poses(X0)
    s0, Xa = ctx.gn_run(V)
    n0 = ctx.gn_factorizations()
    ctx.gn_set_poses(X0)
    c = ctx.gn_marginals()
    assert c.tobytes() == a.tobytes()
    s1, Xb = ctx.gn_run(V)
    assert Xa.tobytes() == Xb.tobytes()
    assert s1["iterations"] == s0["iterations"] and ctx.gn_factorizations() == n0
    assert s1["final_error"] == s0["final_error"]


def test_errors_write_nothing(ctx):
    """DPG_ERR_ARG / DPG_ERR_STATE cases; the output buffer keeps its sentinel in every one."""
    import ctypes as C
    from dpgslam import _abi, api
    from dpgslam._abi import lib, ptr
    X, F = chain_graph(V=12)
    V = len(X)
    sent = 12345.678

    def raw_nodes(c, nodes, n=None):
        nd = np.asarray(nodes, np.int32)
        out = np.full((max(len(nd), 1), 9), sent)
        rc = lib().dpg_gn_marginals(c.handle, ptr(nd, C.c_int32), len(nd) if n is None else n, ptr(out, C.c_double))
        assert np.all(out == sent)
        return rc

    def raw_pairs(c, pairs):
        pr = np.asarray(pairs, np.int32).reshape(-1, 2)
        out = np.full((len(pr), 9), sent)
        rc = lib().dpg_gn_marginal_pairs(c.handle, ptr(pr, C.c_int32), len(pr), ptr(out, C.c_double))
        assert np.all(out == sent)
        return rc

    ctx.gn_setup(V, F)
    ctx.gn_set_poses(X)
    assert raw_nodes(ctx, [0, V]) == ARG
    assert raw_nodes(ctx, [3, -1]) == ARG
    assert raw_pairs(ctx, [(0, 1), (4, 6)]) == ARG        # (i, i + 2) of a chain shares no factor
    assert raw_pairs(ctx, [(0, V)]) == ARG
    with pytest.raises(_abi.DpgError) as e:
        ctx.gn_marginals([V])
    assert err_code(e) == ARG
    with pytest.raises(_abi.DpgError) as e:
        ctx.gn_marginal_pairs([(3, 5)])
    assert err_code(e) == ARG
    assert np.all(np.isfinite(ctx.gn_marginals([0, V - 1])))
    # no Cholesky: the graph was set up for PCG
    gp = _abi.default_gn_params()
    gp.linear_solver = _abi.DPG_SOLVER_PCG
    ctx.gn_setup(V, F, params=gp)
    ctx.gn_set_poses(X)
    assert raw_nodes(ctx, [0]) == STATE
    assert raw_pairs(ctx, [(0, 1)]) == STATE
    ctx.gn_setup(V, F)
    # before any setup
    with api.Context(0) as fresh:
        assert raw_nodes(fresh, [0]) == STATE
        with pytest.raises(_abi.DpgError) as e:
            fresh.gn_marginals()
        assert err_code(e) == STATE
    # more than one rank
    with api.Context(0, virtual=2) as two:
        two.gn_setup(V, F)
        two.gn_set_poses(X)
        assert raw_nodes(two, [0]) == STATE
        out = np.full((V, 9), sent)
        rc = lib().dpg_marginal_covariances(two.handle, ptr(np.ascontiguousarray(X), C.c_double), V,
                                            F.ctypes.data_as(C.c_void_p), len(F), None, V, ptr(out, C.c_double))
        assert rc == STATE and np.all(out == sent)


def _inc_sequence(ctx, X0, F, with_marginals, full_refactor=False, checks=()):
    """One node per update with its factors to earlier nodes; returns the estimates after every
    update and the marginals (with the exported state) after the updates in `checks`."""
    from dpgslam import api
    g = api.IncGraph(ctx, mode="isam2", reorder_every=8, full_refactor=full_refactor)
    last = np.maximum(F["i"], np.where(F["kind"] == BETWEEN, F["j"], 0))
    est, marg = [], {}
    try:
        for v in range(len(X0)):
            g.update(X0[v:v + 1], F[last == v])
            if with_marginals and (v + 1) in checks:
                marg[v + 1] = (g.marginals(), g.export_state())
            est.append(g.poses().copy())
    finally:
        g.close()
    return est, marg


def test_incremental_graph(ctx):
    """ISAM2-mode updates with reorders and moved fronts: the marginals match H^-1 at theta, are
    bitwise those of full refactorizations, and leave the estimates bitwise alone."""
    X0, F, _ = consistent_mesh_graph(V=64, k=6)
    keep = (F["i"] < 60) & ((F["kind"] != BETWEEN) | (F["j"] < 60))
    X0, F = X0[:60], F[keep]
    checks = (5, 17, 33, 60)
    est_a, marg_a = _inc_sequence(ctx, X0, F, True, checks=checks)
    assert sorted(marg_a) == list(checks)
    for k in checks:
        got, stt = marg_a[k]
        assert got.shape == (k, 3, 3) and len(stt["theta"]) == k
        S, tol = dense_reference(f"inc60@{k}", stt["factors"], stt["theta"])
        check_nodes(f"inc60@{k}", got, S, tol)
    _, marg_b = _inc_sequence(ctx, X0, F, True, full_refactor=True, checks=checks)
    for k in checks:
        assert marg_a[k][0].tobytes() == marg_b[k][0].tobytes(), k
    est_c, _ = _inc_sequence(ctx, X0, F, False)
    for a, c in zip(est_a, est_c):
        assert a.tobytes() == c.tobytes()


def test_slam_get_pose_covariance():
    """DpgSLAM.GetPoseCovariance over a short synthetic session (tests/test_slam.py's)."""
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
        cov = s.GetPoseCovariance()
        assert cov.shape == (3, 3) and np.array_equal(cov, cov.T)
        assert np.linalg.eigvalsh(cov).min() > 0.0
        assert np.array_equal(cov, s.be.inc.marginals([V - 1])[0])
        assert np.array_equal(s.GetPoseCovariance(2), s.be.inc.marginals([2])[0])
        with pytest.raises(IndexError):
            s.GetPoseCovariance(V)
