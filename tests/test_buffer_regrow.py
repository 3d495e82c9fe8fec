"""Regrowth of the buffers the solver, the incremental graph, the DPG store and the context's batch
graph own (csrc/dpg_buf.h: OwnedBuf behind DevBuf / PinBuf) while every lazily created buffer exists:
results must not depend on how often, or in what state, an array was reallocated or a graph replaced.

The incremental graph is compared with OracleIncGraph (poses, tests/test_inc.py's bound) and with the
dense inverse of the oracle's H at the oracle's linearization points (tests/test_marginals.py's
reference and tolerance rule); the store with a store that was created whole, exactly."""
import math

import numpy as np
import pytest

from graphs import pose_diff
from oracle import oracle as O
from multi_common import perr
from test_ctx_teardown import _two_node_graph
from test_inc import POSE_TOL
from test_marginals import blk, dense_reference, rel_err, rel_pose

pytestmark = pytest.mark.gpu

V_END = 48
CHECKS = (3, 12, 48)


def _loop_chain(V=V_END, seed=11):
    """Exactly consistent chain with a loop closure (v - 6, v) at every 6th node and a prior on node
    0; initial values within 0.03 of the truth, so no |delta| reaches ISAM2's relinearization
    threshold (0.1) and the linearization points stay the initial values, bit for bit, on both sides.
    Returns (X0, factors by arriving node)."""
    from dpgslam import api
    rng = np.random.default_rng(seed)
    X = np.column_stack([np.cumsum(rng.uniform(0.5, 1.0, V)), rng.normal(0, 0.3, V), rng.uniform(-1.0, 1.0, V)])
    X0 = X + rng.uniform(-0.03, 0.03, X.shape)
    sig = (0.1, 0.1, 0.05)
    by_node = {v: [] for v in range(V)}
    by_node[0].append(api.prior_factor(0, tuple(X[0]), sig))
    for v in range(1, V):
        by_node[v].append(api.between_factor(v - 1, v, rel_pose(X, v - 1, v), sig))
        if v % 6 == 0:
            by_node[v].append(api.between_factor(v - 6, v, rel_pose(X, v - 6, v), sig))
    return X0, {v: np.concatenate(f) for v, f in by_node.items()}


def _pairs(V):
    """Five pairs of nodes that share no factor, both orientations among them (V = 3 has only (0, 2)
    and (2, 0) to cycle through)."""
    far = [(i, j) for i in range(V) for j in range(V) if abs(i - j) >= 2 and not (abs(i - j) == 6 and max(i, j) % 6 == 0)]
    pick = np.linspace(0, len(far) - 1, 5).astype(int)
    return [far[q] for q in pick]


def _joint_nodes(V):
    return [0, V - 1, V // 2]


def _run(g, X0, by_node, oracle=None):
    """Nodes 0 and 1 in the first update, then one node per update; at every V in CHECKS all
    marginals, five cross-covariances and one joint marginal.  With an oracle, it runs in lockstep
    and the results are checked against it."""
    out = []
    for v in range(1, len(X0)):
        x = X0[:2] if v == 1 else X0[v:v + 1]
        f = np.concatenate([by_node[0], by_node[1]]) if v == 1 else by_node[v]
        g.update(x, f)
        V = v + 1
        assert g.V == V
        if oracle is not None:
            oracle.update(x, f)
        rec = [g.poses().copy()]
        if V in CHECKS:
            pr, jn = _pairs(V), _joint_nodes(V)
            rec += [g.marginals(), g.cross_covariances(pr), g.joint_marginal(jn)]
            if oracle is not None:
                assert np.array_equal(g.export_state()["theta"], oracle.theta)
                d = np.abs(pose_diff(rec[0], oracle.poses())).max()
                jp = [(a, b) for a in jn for b in jn]
                S, tol = dense_reference(f"regrow48@{V}", oracle.F, oracle.theta, pairs=pr + jp)
                errs = [rel_err(rec[1][i], blk(S, i, i)) for i in range(V)]
                errs += [rel_err(rec[2][q], blk(S, i, j)) for q, (i, j) in enumerate(pr)]
                errs += [rel_err(blk(rec[3], a, b), blk(S, jn[a], jn[b])) for a in range(3) for b in range(3)]
                print(f"[regrow48@{V}] poses {d:.3g} (bound {POSE_TOL:g})  max block error {max(errs):.3g} (tol {tol:.3g})")
                assert d < POSE_TOL, (V, d)
                assert max(errs) <= tol, (V, max(errs), tol)
        out.append(rec)
    if oracle is not None:
        d = np.abs(pose_diff(g.poses(), oracle.poses())).max()
        assert d < POSE_TOL, d
    return out


def test_inc_regrow_with_optional_buffers(ctx):
    """46 one-node updates rebuild the solver 46 times (reorder_every 4) and regrow each of its
    arrays several times under the 1.5x rule, with the selected inverse's, the picks' and the joint
    marginals' buffers alive from V = 3 on and re-prepared against new analyses at V = 12 and 48.
    After reset() the same sequence on the same object -- every buffer now at its final capacity --
    gives the same poses and covariances bit for bit."""
    from dpgslam import api
    X0, by_node = _loop_chain()
    g = api.IncGraph(ctx, mode="isam2", reorder_every=4)
    try:
        first = _run(g, X0, by_node, O.OracleIncGraph(mode="isam2"))
        assert sum(len(r) == 4 for r in first) == len(CHECKS)
        g.reset()
        assert g.V == 0
        again = _run(g, X0, by_node)
    finally:
        g.close()
    for v, (a, b) in enumerate(zip(first, again)):
        assert len(a) == len(b)
        for q, (x, y) in enumerate(zip(a, b)):
            assert x.tobytes() == y.tobytes(), (v + 2, q)


def _scans(n=32, seed=4):
    """2 scans of 16 beams, then 30 with beam counts cycling through 2, 16, 33; poses along a short arc."""
    rng = np.random.default_rng(seed)
    nb = [16, 16] + [(2, 16, 33)[k % 3] for k in range(n - 2)]
    off = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
    ranges = rng.uniform(2.0, 6.0, int(off[-1])).astype(np.float32)
    geom = np.tile(np.array([-math.pi, math.pi, 8.0], np.float32), (n, 1))
    t = np.arange(n, dtype=np.float32)
    est = np.column_stack([0.15 * t, 0.4 * np.sin(0.3 * t), 0.05 * t]).astype(np.float32)
    return off, ranges, geom, est


def _same_grid(a, b):
    assert (a["width"], a["height"], a["origin"], a["resolution"]) == (b["width"], b["height"], b["origin"], b["resolution"])
    assert a["data"].tobytes() == b["data"].tobytes()
    assert a["hits"].tobytes() == b["hits"].tobytes() and a["misses"].tobytes() == b["misses"].tobytes()


def test_store_append_regrows_everything(ctx):
    """A store grown from 2 scans by 30 one-scan appends (2, 16 and 33 beams in turn: the device
    arrays, the pinned mirrors and the append staging are all reallocated repeatedly, the grid and
    geometry buffers existing from the 3rd append on) equals a store created with all 32 scans:
    grids and beam geometry after the 3rd and the last append, then labels, sectors, activity, the
    grid and the geometry after one executeDPG, exactly."""
    from dpgslam import api
    off, ranges, geom, est = _scans()
    n = len(off) - 1
    whole = api.DpgStore(ctx, ranges, geom, offsets=off)
    grown = api.DpgStore(ctx, ranges[:off[2]], geom[:2], offsets=off[:3])
    try:
        for v in range(2, n):
            grown.append(ranges[off[v]:off[v + 1]], geom[v:v + 1], offsets=off[v:v + 2] - off[v])
            if v + 1 in (5, n):
                V = v + 1
                _same_grid(grown.occupancy_grid(V, est[:V], counts=True), whole.occupancy_grid(V, est[:V], counts=True))
                for a, b in zip(grown.beam_geometry(V, est[:V]), whole.beam_geometry(V, est[:V])):
                    assert a.shape == b.shape and a.tobytes() == b.tobytes()
        assert grown.V == whole.V == n and np.array_equal(grown.offsets, whole.offsets)
        sg, sw = grown.execute_dpg(n, 6, est), whole.execute_dpg(n, 6, est)
        assert sg.counters() == sw.counters()
        for a, b in zip(grown.fetch(), whole.fetch()):
            assert a.tobytes() == b.tobytes()
        _same_grid(grown.occupancy_grid(n, est, counts=True), whole.occupancy_grid(n, est, counts=True))
        for a, b in zip(grown.beam_geometry(n, est), whole.beam_geometry(n, est)):
            assert a.tobytes() == b.tobytes()
    finally:
        grown.close()
        whole.close()


def _batch_graphs():
    """(X0, F) of the two-node graph of tests/test_ctx_teardown.py, the 12-node loop chain and a three-node chain."""
    out = [_two_node_graph()[:2]]
    for V in (12, 3):
        X0, by_node = _loop_chain(V)
        out.append((X0, np.concatenate([by_node[v] for v in range(V)])))
    return out


def _gn(c, X0, F):
    c.gn_setup(len(X0), F)
    c.gn_set_poses(X0)
    return c.gn_run(len(X0))[1]


def test_batch_graph_replaced_on_one_context():
    """Three graphs set up in turn on ONE context, each replacing the last (the 12-node one with the
    solver's selected-inverse buffers alive), then a setup that fails: every graph's poses equal, byte
    for byte, those of a fresh context given only that graph, and the failed setup leaves the
    three-node graph live -- a run from its initial poses gives its bytes again."""
    from dpgslam import _abi, api
    graphs = _batch_graphs()
    fresh = []
    for X0, F in graphs:
        with api.Context(0) as c:
            fresh.append(_gn(c, X0, F).tobytes())
    with api.Context(0) as c:
        for (X0, F), want in zip(graphs, fresh):
            assert _gn(c, X0, F).tobytes() == want, len(X0)
            if len(X0) == 12:
                assert c.gn_marginals().shape == (12, 3, 3)
        X0, F = graphs[-1]
        bad = api.between_factor(0, len(X0), (1.0, 0.0, 0.0), (0.1, 0.1, 0.05))   # j == V
        with pytest.raises(_abi.DpgError, match=r"\(-1\)"):   # DPG_ERR_ARG
            c.gn_setup(len(X0), np.concatenate([F, bad]))
        c.gn_set_poses(X0)
        assert c.gn_run(len(X0))[1].tobytes() == fresh[-1]


def test_virtual_devices_graph_replaced():
    """optimize_graph on two virtual devices for the 12-node graph, the two-node graph and the 12-node
    graph again: every setup regrows hb_own by the vote words and makes hb_part and the ownership
    bytes anew.  tests/test_multi_gpu_ctx.py's bar against one device (the same iteration and
    factorization counts, poses within 1e-9); the first and the third result byte-identical."""
    from dpgslam import api
    two, twelve, _ = _batch_graphs()
    ref = {}
    for X0, F in (two, twelve):
        with api.Context(0) as c:
            X, st = c.optimize_graph(X0, F)
            ref[len(X0)] = (X, st.iterations, c.gn_factorizations())
    got = []
    with api.Context(0, virtual=2) as c:
        for X0, F in (twelve, two, twelve):
            X, st = c.optimize_graph(X0, F)
            Xr, it, nf = ref[len(X0)]
            assert (st.iterations, c.gn_factorizations()) == (it, nf), len(X0)
            assert perr(X, Xr) < 1e-9, (len(X0), perr(X, Xr))
            got.append(X.tobytes())
    assert got[0] == got[2]
