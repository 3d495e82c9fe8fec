"""Numpy restatement of the loop-closure verification (the contract above dpg_verify_params in
include/dpg_slam_c.h), sharing no code with the kernel: the sensor key, the OCC and FREE cells of a
model cloud, the moved points of both directions, the counts and the result record.  Keys and the C
round come from tests/csm_ref.py; everything after the float32 transform is integer."""
import numpy as np

from csm_ref import c_round, keys  # noqa: F401  (c_round: for the tests that pin it)
from dpgslam import _abi

f32 = np.float32


def sensor_key(p):
    """(ax, ay): the key of the params' sensor position."""
    kx, ky, ok = keys(np.array([[p.sensor[0], p.sensor[1]]], f32), p.resolution)
    assert ok.all()
    return int(kx[0]), int(ky[0])


def ray_offsets(d, n, i):
    """off(d, n, i) = sign(d) floor((2 i |d| + n) / (2 n)), int64 arrays (or Python ints)."""
    d, n, i = np.asarray(d, np.int64), np.asarray(n, np.int64), np.asarray(i, np.int64)
    return np.sign(d) * ((2 * i * np.abs(d) + n) // (2 * n))


def free_cells(a, b, max_steps=None):
    """The FREE cells of one ray from sensor key a to point key b, unclipped: a list of (u, v) keys for
    i = 0 .. min(n, max_steps) - 1 (max_steps None: all n of them)."""
    dx, dy = int(b[0]) - int(a[0]), int(b[1]) - int(a[1])
    n = max(abs(dx), abs(dy))
    steps = n if max_steps is None else min(n, int(max_steps))
    out = []
    for i in range(steps):
        ox = (1 if dx > 0 else -1 if dx < 0 else 0) * ((2 * i * abs(dx) + n) // (2 * n))
        oy = (1 if dy > 0 else -1 if dy < 0 else 0) * ((2 * i * abs(dy) + n) // (2 * n))
        out.append((int(a[0]) + ox, int(a[1]) + oy))
    return out


def table(cloud, p, max_steps=None):
    """The state of every cell, uint8 [2H + 1, 2H + 1] indexed [v + H, u + H]: 2 occupied, 1 free, 0
    unknown.  max_steps None: the contract's min(n, 2H + 1) steps per ray; else min(n, max_steps)."""
    H, R = int(p.half_cells), int(p.occ_radius)
    W = 2 * H + 1
    ax, ay = sensor_key(p)
    assert abs(ax) <= H and abs(ay) <= H
    kx, ky, ok = keys(cloud, p.resolution)
    kx, ky = kx[ok], ky[ok]
    occ = np.zeros((W, W), bool)
    free = np.zeros((W, W), bool)
    for oy in range(-R, R + 1):
        for ox in range(-R, R + 1):
            if ox * ox + oy * oy > R * R:
                continue
            u, v = kx + ox + H, ky + oy + H
            m = (u >= 0) & (u < W) & (v >= 0) & (v < W)
            occ[v[m], u[m]] = True
    dx, dy = kx - ax, ky - ay
    n = np.maximum(np.abs(dx), np.abs(dy))
    steps = np.minimum(n, W if max_steps is None else int(max_steps))
    for i in range(int(steps.max(initial=0))):
        m = i < steps
        u = ax + ray_offsets(dx[m], n[m], i) + H
        v = ay + ray_offsets(dy[m], n[m], i) + H
        k = (u >= 0) & (u < W) & (v >= 0) & (v < W)
        free[v[k], u[k]] = True
    return np.where(occ, 2, np.where(free, 1, 0)).astype(np.uint8)


def moved(points, T, direction):
    """The moving cloud under T, float32 [N, 2].  Direction 0: q = ((c x) - (s y)) + tx, ((s x) + (c y)) + ty;
    direction 1: d = (x - tx, y - ty), q = (c dx) + (s dy), (c dy) - (s dx); one rounding per operation."""
    pts = np.asarray(points, f32).reshape(-1, 2)
    T = np.asarray(T, f32).reshape(6)
    c, s, tx, ty = T[0], T[3], T[2], T[5]
    x, y = pts[:, 0], pts[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        if direction == 0:
            qx = ((c * x) - (s * y)) + tx
            qy = ((s * x) + (c * y)) + ty
        else:
            dx, dy = x - tx, y - ty
            qx = (c * dx) + (s * dy)
            qy = (c * dy) - (s * dx)
    assert qx.dtype == f32 and qy.dtype == f32
    return np.stack([qx, qy], 1)


def counts(tbl, q, p):
    """(n_pts, n_in, n_support, n_free) of moved points q [N, 2] on the table `tbl`."""
    H = int(p.half_cells)
    kx, ky, ok = keys(q, p.resolution)
    m = ok & (np.abs(kx) <= H) & (np.abs(ky) <= H)
    st = tbl[ky[m] + H, kx[m] + H]
    return len(q), int(m.sum()), int((st == 2).sum()), int((st == 1).sum())


def result(tgt, src, T, p, tables=None):
    """The dpg_verify_result record of one pair (a VERIFY_RESULT_DTYPE scalar).  tables: (the target's,
    the source's) when the caller has them already."""
    tt, ts = tables if tables is not None else (table(tgt, p), table(src, p))
    r = np.zeros((), _abi.VERIFY_RESULT_DTYPE)
    for d, (tbl, mov) in enumerate(((tt, src), (ts, tgt))):
        k = counts(tbl, moved(mov, T, d), p)
        r["n_pts"][d], r["n_in"][d], r["n_support"][d], r["n_free"][d] = k
    r["status"] = _abi.DPG_VERIFY_NO_OVERLAP if (r["n_in"] == 0).any() else _abi.DPG_VERIFY_OK
    return r
