"""dpg_ctx_destroy on a context whose children are still alive.  Python's Context.close closes the
DPG stores and incremental graphs first, so the C side's own order -- children (newest first),
peers, communicators, the drained stream, the collective thread, then the context's device arrays
-- only runs when a C caller, or a finalizer that reached the context first, destroys the raw
handle."""
import numpy as np
import pytest


def _two_node_graph():
    """A prior on node 0 and one exactly consistent Between: the optimum is x0 = 0, x1 = (2, 0, 0)."""
    from dpgslam import api
    F = np.concatenate([api.prior_factor(0, (0.0, 0.0, 0.0), (0.3, 0.3, 0.1)),
                        api.between_factor(0, 1, (2.0, 0.0, 0.0), (0.2, 0.2, 0.1))])
    X0 = np.array([[0.3, -0.1, 0.1], [2.2, 0.1, -0.1]])
    X_opt = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    return X0, F, X_opt


@pytest.mark.gpu
def test_destroy_with_live_children_then_fresh_context():
    from dpgslam import api
    from graphs import pose_diff
    X0, F, X_opt = _two_node_graph()
    ctx = api.Context(0)
    inc = api.IncGraph(ctx)
    inc.update(X0, F)
    assert inc.V == 2
    ranges = np.full((2, 16), 5.0, np.float32)
    geom = np.tile(np.array([-np.pi, np.pi, 8.0], np.float32), (2, 1))
    store = api.DpgStore(ctx, ranges, geom)
    # the raw handle goes while both children live: the context destroys them itself
    api.lib().dpg_ctx_destroy(ctx.handle)
    ctx.handle = None
    for child in (inc, store):
        child.close()   # nothing left to destroy: only the dangling handle is dropped
        assert child.handle is None
    ctx.close()
    with api.Context(0) as fresh:
        X, st = fresh.optimize_graph(X0, F)
        # zero-residual optimum, fp64 Gauss-Newton to its default step tolerance (as smoke())
        assert st.iterations > 0 and np.abs(pose_diff(X, X_opt)).max() < 1e-9, X


@pytest.mark.gpu
def test_destroy_with_every_lazy_resource_allocated():
    """The same with everything that is created on first use in existence: the solver's selected
    inverse, pick and joint-marginal buffers (marginals and a joint marginal of the incremental
    graph), the store's grid buffers (an occupancy grid) and, on the context's own graph, L11^-1
    with the stream and events it is computed on (a batch solve with solve_inv_cols = 1).  Each owner
    releases what it holds; a fresh context then solves as before."""
    from dpgslam import api
    from graphs import pose_diff
    X0, F, X_opt = _two_node_graph()
    ctx = api.Context(0)
    inc = api.IncGraph(ctx)
    inc.update(X0, F)
    assert inc.marginals().shape == (2, 3, 3) and inc.joint_marginal([1, 0]).shape == (6, 6)
    ranges = np.full((2, 16), 5.0, np.float32)
    geom = np.tile(np.array([-np.pi, np.pi, 8.0], np.float32), (2, 1))
    store = api.DpgStore(ctx, ranges, geom)
    assert (store.occupancy_grid(2, np.zeros((2, 3), np.float32))["data"] == 100).any()
    ctx.set_solver_options(solve_inv_cols=1)
    X, st = ctx.optimize_graph(X0, F)
    assert st.iterations > 0 and np.abs(pose_diff(X, X_opt)).max() < 1e-9, X
    api.lib().dpg_ctx_destroy(ctx.handle)
    ctx.handle = None
    for child in (inc, store):
        child.close()
        assert child.handle is None
    ctx.close()
    with api.Context(0) as fresh:
        X, st = fresh.optimize_graph(X0, F)
        assert st.iterations > 0 and np.abs(pose_diff(X, X_opt)).max() < 1e-9, X


@pytest.mark.gpu
def test_destroy_virtual_context_with_every_lazy_resource(workload):
    """Two virtual devices with everything a context makes on first use in existence: a batch with its
    covariance on the side stream (config1), the map events (one get_map), and -- optimize_graph --
    the pipelined loop's control block and report slots and the ownership buffers on both device
    contexts.  The raw destroy releases all of it; a fresh context then solves as before."""
    from dpgslam import _abi, api
    from graphs import pose_diff
    X0, F, X_opt = _two_node_graph()
    w = workload("config1")
    p = _abi.default_icp_params()
    ctx = api.Context(0, virtual=2)
    ctx.upload_scans(w.pts, w.offsets, p.downsample_icp_points_ratio)
    res, hess = ctx.icp_batch(w.edges, w.est, p, compute_cov=True)
    assert len(res) == w.E and np.isfinite(hess).all()
    assert len(ctx.get_map(w.est)) > 0
    X, st = ctx.optimize_graph(X0, F)
    assert st.iterations > 0 and np.abs(pose_diff(X, X_opt)).max() < 1e-9, X
    api.lib().dpg_ctx_destroy(ctx.handle)
    ctx.handle = None
    ctx.close()
    with api.Context(0) as fresh:
        X, st = fresh.optimize_graph(X0, F)
        assert st.iterations > 0 and np.abs(pose_diff(X, X_opt)).max() < 1e-9, X
