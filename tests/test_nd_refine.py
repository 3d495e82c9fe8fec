"""The nested dissection's vertex-separator refinement (dpg_chol_sym.cpp, nd_refine): its host-side
properties on the smallest graphs at which it can go wrong (tools/nd_refine_check.cpp), and the
automatic order -- which may now be a refined one -- against round 2's order and minimum degree on
a graph just past the automatic rule's 256-node threshold."""
import math
import os
import subprocess

import numpy as np
import pytest

from graphs import pose_diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_separator_refinement_properties(tmp_path):
    """A fat grid separator shrinks to one column's size and stays a balanced separator, a ladder's
    root separator is at most 2 nodes, a clique with pendant chains keeps both sides, the refined
    orders repeat and their threaded form equals the serial one, refine = 0 gives the order from
    before the refinement, every order is a permutation.  Built with DPG_ND_VERIFY every refined
    split is checked to separate."""
    out = str(tmp_path / "nd_refine_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-DDPG_ND_VERIFY", "-o", out,
                    os.path.join(ROOT, "tools", "nd_refine_check.cpp"),
                    os.path.join(ROOT, "dpg-slam_amd", "csrc", "dpg_chol_sym.cpp")], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr


def ladder_graph(L=200, closures=6, seed=3):
    """A route driven out and back (2 x L nodes, 1 m steps, the return leg 1 m beside the first):
    the odometry chain, a rung between the two legs at every step and a few long-range closures.
    Exact relative measurements plus noise.  Returns (X0, factors)."""
    from dpgslam import api
    rng = np.random.default_rng(seed)
    V = 2 * L
    X = np.zeros((V, 3))
    X[:L, 0] = np.arange(L)
    X[L:, 0] = np.arange(L)[::-1]
    X[L:, 1] = 1.0
    X[L:, 2] = math.pi
    X[:, 2] += rng.uniform(-0.3, 0.3, V)

    def rel(i, j):   # Pose2 between: Xi^-1 Xj
        c, s = math.cos(X[i, 2]), math.sin(X[i, 2])
        dx, dy = X[j, 0] - X[i, 0], X[j, 1] - X[i, 1]
        d = X[j, 2] - X[i, 2]
        return np.array([c * dx + s * dy, -s * dx + c * dy, math.atan2(math.sin(d), math.cos(d))])

    pairs = set((i, i + 1) for i in range(V - 1))
    pairs |= set((i, V - 1 - i) for i in range(L - 1))
    while len(pairs) < V - 1 + L - 1 + closures:
        i, j = sorted(int(v) for v in rng.integers(0, V, 2))
        if j - i > 20:
            pairs.add((i, j))
    sig = np.array([0.05, 0.05, 0.02])
    F = [api.prior_factor(0, tuple(X[0]), (0.1, 0.1, 0.05))]
    for i, j in sorted(pairs):
        F.append(api.between_factor(i, j, tuple(rel(i, j) + rng.normal(0, 1, 3) * sig), tuple(sig)))
    X0 = X + rng.normal(0, 1, X.shape) * np.array([0.1, 0.1, 0.05])
    return X0, np.concatenate(F)


@pytest.mark.gpu
def test_ladder_orders_agree(ctx):
    """A 2 x 200 ladder with long-range closures (400 nodes: the automatic rule picks among its
    candidate orders, the refined ones included) solved under the automatic order, round 2's
    nested dissection and minimum degree: the same iteration count and the same poses to 1e-9."""
    from dpgslam import _abi
    X0, F = ladder_graph()

    def solve(**solver):
        ctx.set_solver_options(**solver)
        try:
            return ctx.optimize_graph(X0, F, _abi.default_gn_params())
        finally:
            ctx.set_solver_options()

    Xa, sa = solve()
    Xn, sn = solve(order="nd")
    Xm, sm = solve(order="md")
    assert sa.iterations == sn.iterations == sm.iterations
    assert sa.iterations > 1
    assert np.abs(pose_diff(Xa, Xn)).max() < 1e-9
    assert np.abs(pose_diff(Xa, Xm)).max() < 1e-9
