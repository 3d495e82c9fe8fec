"""The batched ICP kernels on the adversarial clouds of icp_cases.py, against the oracle.

The synthetic scans of the other GPU tests are near-uniform rooms at a handful of sizes and one set
of parameters.  Here: clouds on and next to every switch between the angular kernel's forms (and of
1 .. 4 points: shorter than a trip of candidates, where the repeated records wrap), unequal pairs
in one batch, exact distance ties and duplicates, points on the pseudo-angle's octant seams and at
the origin, collinear rays across the bucket table's wrap, clouds a few cm from the origin and
100 m out, the correspondence distance from 0.02 to 10, no reciprocity, one and two required
correspondences, failing alignments, and empty clouds -- under every nearest-neighbour variant,
angular kernel form and cooperative-queue threshold.  Everything is byte equality (results, and
per-iteration correspondences where a wrong tie order could still converge to the same transform);
the one tolerance is the covariance block's existing bar.  test_icp_adversarial_cpu.py pins the
oracle side of every case."""
import numpy as np
import pytest

import icp_cases as C

pytestmark = pytest.mark.gpu

FIELDS = ("T", "z", "converged", "iterations", "n_corr", "status", "fitness")
NN_VARIANTS = ("angular", "kdtree", "grid")
DEFER_CAPS = (0, 1, 8, 256)
DEFER_DEFAULT = 256
TRACED_GROUPS = ("ties", "angles", "mixed")
DEFER_CASES = ["range/near_r0.6", "range/near_r0.05", "angles/ray_px", "angles/ray_nx", "angles/ray_diag",
               "sizes/n512", "sizes/n1024", "sizes/n2048", "sizes/n4096", "sizes/n8192", "sizes/n16384",
               "mixed/all", "ties/half_x", "ties/dup_reversed"]
_REF = {}
_REF_TRACE = {}


def _ref(c):
    """The oracle's results and covariance blocks of a case, computed once."""
    from oracle import oracle as O
    if c.name not in _REF:
        _REF[c.name] = O.icp_batch(c.pts, c.offsets, c.edges, c.est, c.params(), O.NN_GRID, threads=16)
    return _REF[c.name]


def _ref_trace(c, e):
    """The oracle's correspondences of edge e, [TRACE_ITERS, n_src] (grid search: the CPU test has it
    equal to brute force on every case)."""
    from oracle import oracle as O
    if (c.name, e) not in _REF_TRACE:
        t, s = c.edges[e]
        sd, td = O.downsample(c.cloud(s), c.ratio), O.downsample(c.cloud(t), c.ratio)
        _REF_TRACE[(c.name, e)] = O.icp_align(sd, td, O.icp_guess(c.est[s], c.est[t]), c.params(), O.NN_GRID,
                                              trace_iters=C.TRACE_ITERS)[1]
    return _REF_TRACE[(c.name, e)]


def _same(res, ref, what):
    """test_icp_large._same, naming the case."""
    for k in FIELDS:
        a, b = np.asarray(res[k]), np.asarray(ref[k])
        bad = np.nonzero(~np.all((a == b).reshape(len(a), -1), axis=1))[0]
        assert len(bad) == 0, f"{what}: {k} differs on edges {bad[:8]}: {a[bad[:3]]} vs {b[bad[:3]]}"
        assert a.tobytes() == b.tobytes(), f"{what}: {k} equal as numbers, not as bytes (a signed zero)"


def _n_src(c, e):
    s = c.edges[e, 1]
    return (int(c.offsets[s + 1] - c.offsets[s]) + c.ratio - 1) // c.ratio


def _traced_edges(c):
    """The edges whose per-iteration correspondences are compared."""
    if c.group in TRACED_GROUPS:
        return list(range(len(c.edges)))
    if c.group == "sizes":
        n = np.diff(c.offsets)
        return [e for e, (t, s) in enumerate(c.edges) if max(n[t], n[s]) <= 65]
    return []


def _same_trace(ctx, c, ref, what):
    edges = _traced_edges(c)
    if not edges:
        return
    tr = ctx.icp_fetch_trace(C.TRACE_ITERS)
    for e in edges:
        n, ns = min(int(ref["iterations"][e]), C.TRACE_ITERS), _n_src(c, e)
        rt = _ref_trace(c, e)
        bad = np.argwhere(tr[e, :n, :ns] != rt[:n])
        assert len(bad) == 0, (f"{what}: edge {e} correspondences differ first at iteration {bad[0][0]}, source point "
                               f"{bad[0][1]}: {tr[e, bad[0][0], bad[0][1]]} vs {rt[bad[0][0], bad[0][1]]}")


def _run(ctx, c, what, compute_cov=False):
    """The case's batch on the context as it is set; results checked against the oracle (and the
    correspondences where the case is traced).  Returns (results, covariance blocks)."""
    ref, _ = _ref(c)
    trace = C.TRACE_ITERS if _traced_edges(c) else 0
    res, hess = ctx.icp_batch(c.edges, c.est, c.params(), compute_cov=compute_cov, trace_iters=trace)
    _same(res, ref, what)
    if trace:
        _same_trace(ctx, c, ref, what)
    return res, hess


def _all_variants(ctx, c):
    """Every NN variant that takes the case (the other two must refuse it with DPG_ERR_SIZE) and, under
    the angular one, kernel forms 1 and 2 byte-identical to form 0."""
    from dpgslam import _abi
    try:
        ctx.upload_scans(c.pts, c.offsets, c.ratio)
        for v in NN_VARIANTS:
            ctx.set_icp_variant(v)
            if v != "angular" and c.max_points() > C.KD_GRID_MAX:
                with pytest.raises(_abi.DpgError, match=r"\(-4\)"):   # DPG_ERR_SIZE
                    ctx.icp_batch(c.edges, c.est, c.params(), compute_cov=False)
                continue
            res, _ = _run(ctx, c, f"{c.name} [{v}]")
            if v == "angular":
                for kv in (1, 2):
                    ctx.set_icp_kernel_variant(kv)
                    res_kv, _ = _run(ctx, c, f"{c.name} [angular, kernel form {kv}]")
                    assert res_kv.tobytes() == res.tobytes(), f"{c.name}: kernel form {kv} differs from form 0"
                ctx.set_icp_kernel_variant(0)
    finally:
        ctx.set_icp_kernel_variant(0)
        ctx.set_icp_variant("angular")


@pytest.mark.parametrize("name", C.all_names(("sizes", "mixed", "ties", "angles", "range", "params", "ratio")))
def test_adversarial_bit_exact(ctx, name):
    _all_variants(ctx, C.case(name))


@pytest.mark.parametrize("name", DEFER_CASES)
def test_defer_cap_identical(ctx, name):
    """dpg_ctx_set_icp_defer_cap: "results are identical for every value".  Cap 1 queues nearly every
    window, so every iteration overflows the 64-item queue and the rest is scanned in-lane; cap 0
    never queues."""
    c = C.case(name)
    try:
        ctx.upload_scans(c.pts, c.offsets, c.ratio)
        for cap in DEFER_CAPS:
            ctx.set_icp_defer_cap(cap)
            _run(ctx, c, f"{name} [defer cap {cap}]")
    finally:
        ctx.set_icp_defer_cap(DEFER_DEFAULT)


def _record(r):
    from dpgslam import _abi
    return np.frombuffer(bytes(r), _abi.RESULT_DTYPE)


@pytest.mark.parametrize("name,edge", [("mixed/le4096", 0), ("params/one_point_min_corr1", 0), ("params/disjoint", 0),
                                       ("ties/half_x", 0)])
def test_run_icp_matches_batch_and_oracle(ctx, name, edge):
    """The single-alignment entry: the same record as the batch path and the oracle."""
    from dpgslam import _abi, api
    from oracle import oracle as O
    c = C.case(name)
    p = c.params()
    t, s = c.edges[edge]
    ok, z, cov, res, hess = ctx.run_icp(api.Node(c.est[t], c.cloud(t)), api.Node(c.est[s], c.cloud(s)), p,
                                        with_hessian=True)
    ref, _, ref_h = O.run_icp(c.cloud(s), c.cloud(t), c.est[s], c.est[t], p, O.NN_GRID)
    one = _record(res)
    _same(one, _record(ref), f"{name} [run_icp vs oracle]")
    _same(one, _ref(c)[0][edge:edge + 1], f"{name} [run_icp vs the oracle's batch]")
    ctx.upload_scans(c.pts, c.offsets, c.ratio)
    batch, _ = ctx.icp_batch(c.edges, c.est, p, compute_cov=False)
    _same(one, batch[edge:edge + 1], f"{name} [run_icp vs icp_batch]")
    assert ok == (bool(res.converged) and res.status == _abi.DPG_ICP_OK)
    assert ok == (not c.expect_fail)
    assert z == ((float(ref.z[0]), float(ref.z[1])), float(ref.z[2]))
    np.testing.assert_allclose(hess, ref_h, rtol=1e-12, atol=1e-8)


@pytest.mark.parametrize("name", C.all_names(("mixed", "ratio")))
def test_covariance_block_unequal_clouds(ctx, name):
    """The [x, y, yaw] block over min(n_data, n_model) points of the FULL clouds, where the two differ
    in size (and, at ratio 3, from the downsampled ones): the project's bar, rtol 1e-12 / atol 1e-8."""
    c = C.case(name)
    _, ref_h = _ref(c)
    ctx.upload_scans(c.pts, c.offsets, c.ratio)
    _, hess = _run(ctx, c, f"{name} [with covariance]", compute_cov=True)
    n = np.diff(c.offsets)
    np.testing.assert_array_equal(hess[:, 0, 0], 2.0 * np.minimum(n[c.edges[:, 0]], n[c.edges[:, 1]]))
    err = np.abs(hess - ref_h) - 1e-12 * np.abs(ref_h)
    print(f"{name}: covariance block max (|gpu - oracle| - 1e-12 |oracle|) = {err.max():.3e}")
    np.testing.assert_allclose(hess, ref_h, rtol=1e-12, atol=1e-8, err_msg=name)


def test_empty_clouds(ctx):
    """A node without points is a legal upload: an edge with one ends DPG_ICP_TOO_FEW_CORR after no
    iteration with T = the guess (and a zero covariance block), in every variant, next to an
    ordinary edge of the same batch."""
    from dpgslam import _abi
    c = C.case("empty/batch")
    ref, ref_h = _ref(c)
    n = np.diff(c.offsets)
    empty = (n[c.edges[:, 0]] == 0) | (n[c.edges[:, 1]] == 0)
    assert empty.sum() == 4 and (~empty).sum() == 2
    assert np.all(ref["status"][empty] == _abi.DPG_ICP_TOO_FEW_CORR) and np.all(ref["iterations"][empty] == 0)
    assert np.all(ref["converged"][~empty] == 1)
    try:
        ctx.upload_scans(c.pts, c.offsets, c.ratio)
        for v in NN_VARIANTS:
            ctx.set_icp_variant(v)
            res, hess = ctx.icp_batch(c.edges, c.est, c.params(), compute_cov=True, trace_iters=C.TRACE_ITERS)
            _same(res, ref, f"{c.name} [{v}]")
            np.testing.assert_allclose(hess, ref_h, rtol=1e-12, atol=1e-8, err_msg=v)
            assert not hess[empty].any()
            tr = ctx.icp_fetch_trace(C.TRACE_ITERS)
            for e in np.nonzero(~empty)[0]:
                k, ns = min(int(ref["iterations"][e]), C.TRACE_ITERS), _n_src(c, e)
                np.testing.assert_array_equal(tr[e, :k, :ns], _ref_trace(c, e)[:k], err_msg=f"{v} edge {e}")
        ctx.set_icp_variant("angular")
        for kv in (1, 2):
            ctx.set_icp_kernel_variant(kv)
            res_kv, _ = ctx.icp_batch(c.edges, c.est, c.params(), compute_cov=False)
            _same(res_kv, ref, f"{c.name} [angular, kernel form {kv}]")
    finally:
        ctx.set_icp_kernel_variant(0)
        ctx.set_icp_variant("angular")
