"""Numpy restatement of the correlative scan matcher (the contract above dpg_csm_params in
include/dpg_slam_c.h), sharing no code with the kernel: keys, the smoothed table, the score volume,
the winner with its tie order and the result record.  The smoothing bytes and the rotation table
come from the exported host functions (dpg_csm_lut, dpg_csm_rotations), so no libm call is repeated
here; everything else is integer or a float32 operation numpy rounds once.

Also the small synthetic room the scan-matching tests share (ROOM): two scans of a 12 x 9 m room
with three boxes from two known poses, ray-cast in float64 with a fixed seed for the range noise."""
import math

import numpy as np

from dpgslam import _abi, api

f32 = np.float32
LIMIT = 536870912.0   # 2^29


def c_round(x):
    """C round() of float64: halves away from zero (np.round gives halves to even)."""
    x = np.asarray(x, np.float64)
    t = np.trunc(x)
    return (t + np.sign(x) * (np.abs(x - t) >= 0.5)).astype(np.int64)


def keys(pts, res):
    """(kx, ky, valid) of float32 points [N, 2]: key = round((double)v / (double)(float)res); a point
    with a non-finite coordinate or |v / res| >= 2^29 is not valid."""
    p = np.asarray(pts, f32).reshape(-1, 2).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = p / np.float64(f32(res))
        valid = np.isfinite(d).all(1) & (np.abs(d) < LIMIT).all(1)
    k = c_round(np.where(valid[:, None], d, 0.0))
    return k[:, 0], k[:, 1], valid


def table(tgt, p, lut=None):
    """T[v + H, u + H] of the target cloud, uint8 [2H + 1, 2H + 1]."""
    lut = api.csm_lut(p) if lut is None else lut
    H, R = int(p.half_cells), int(p.kernel_radius)
    W = 2 * H + 1
    T = np.zeros((W, W), np.uint8)
    kx, ky, ok = keys(tgt, p.resolution)
    kx, ky = kx[ok], ky[ok]
    for oy in range(-R, R + 1):
        for ox in range(-R, R + 1):
            d2 = ox * ox + oy * oy
            if d2 > R * R:
                continue
            u, v = kx + ox + H, ky + oy + H
            m = (u >= 0) & (u < W) & (v >= 0) & (v < W)
            np.maximum.at(T, (v[m], u[m]), lut[d2])
    return T


def source_keys(src, rot_a, tx, ty, res):
    """Keys of the source points at one angle: q = ((c x) - (s y)) + tx, ((s x) + (c y)) + ty in float32."""
    s_ = np.asarray(src, f32).reshape(-1, 2)
    c, s = f32(rot_a[0]), f32(rot_a[1])
    x, y = s_[:, 0], s_[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        qx = ((c * x) - (s * y)) + f32(tx)
        qy = ((s * x) + (c * y)) + f32(ty)
    assert qx.dtype == f32 and qy.dtype == f32
    return keys(np.stack([qx, qy], 1), res)


def scores(T, src, guess, p, rot=None):
    """The score volume, int32 [2 ha + 1, 2 hy + 1, 2 hx + 1]."""
    g = np.asarray(guess, f32).reshape(6)
    rot = api.csm_rotations(g, p) if rot is None else rot
    H, hx, hy, ha = int(p.half_cells), int(p.half_x), int(p.half_y), int(p.half_a)
    W = 2 * H + 1
    Tp = np.zeros((W + 2, W + 2), np.int64)   # a zero ring: clipped indices land on it
    Tp[1:-1, 1:-1] = T
    dxs, dys = np.arange(-hx, hx + 1), np.arange(-hy, hy + 1)
    vol = np.zeros((2 * ha + 1, len(dys), len(dxs)), np.int64)
    for a in range(2 * ha + 1):
        kx, ky, ok = source_keys(src, rot[a], g[2], g[5], p.resolution)
        kx, ky = kx[ok], ky[ok]
        U = np.clip(kx[:, None] + dxs[None, :] + H, -1, W) + 1     # [N, X]
        V = np.clip(ky[:, None] + dys[None, :] + H, -1, W) + 1     # [N, Y]
        vol[a] = Tp[V[:, :, None], U[:, None, :]].sum(0)
    assert vol.max(initial=0) < 2 ** 31
    return vol.astype(np.int32)


def winner(vol, p):
    """(a, dx, dy) of the highest score; ties by smaller |a - ha|, then dx^2 + dy^2, then a, dy, dx."""
    hx, hy, ha = int(p.half_x), int(p.half_y), int(p.half_a)
    a, iy, ix = np.nonzero(vol == vol.max())
    dx, dy = ix - hx, iy - hy
    order = sorted(zip(np.abs(a - ha), dx * dx + dy * dy, a, dy, dx))
    _, _, ba, bdy, bdx = order[0]
    return int(ba), int(bdx), int(bdy)


def result(tgt, src, guess, p, T=None):
    """The dpg_csm_result record of one pair (a CSM_RESULT_DTYPE scalar) and its score volume."""
    g = np.asarray(guess, f32).reshape(6)
    rot = api.csm_rotations(g, p)
    T = table(tgt, p) if T is None else T
    vol = scores(T, src, g, p, rot)
    a, dx, dy = winner(vol, p)
    res = np.float64(f32(p.resolution))
    r = np.zeros((), _abi.CSM_RESULT_DTYPE)
    c, s = rot[a]
    r["guess"] = [c, -s, f32(np.float64(g[2]) + dx * res), s, c, f32(np.float64(g[5]) + dy * res)]
    r["score"] = vol[a, dy + int(p.half_y), dx + int(p.half_x)]
    r["score_at_guess"] = vol[int(p.half_a), int(p.half_y), int(p.half_x)]
    r["n_src"] = len(np.asarray(src).reshape(-1, 2))
    r["best_a"], r["best_dx"], r["best_dy"] = a, dx, dy
    r["status"] = _abi.DPG_CSM_OK if r["score"] > 0 else _abi.DPG_CSM_NO_OVERLAP
    return r, vol


def guess_of(x, y, th):
    """Guess rows of a relative pose (source in the target's frame), float32 [6]."""
    return np.array([math.cos(th), -math.sin(th), x, math.sin(th), math.cos(th), y], f32)


def guess_pose(g):
    return float(g[2]), float(g[5]), math.atan2(float(g[3]), float(g[0]))


# ------------------------------------------------------------------ the shared room
def _segments():
    segs = [(0, 0, 12, 0), (12, 0, 12, 9), (12, 9, 0, 9), (0, 9, 0, 0)]
    for x0, y0, x1, y1 in ((2.0, 5.5, 3.5, 7.0), (7.5, 1.5, 9.5, 2.5), (8.5, 6.0, 9.5, 7.5)):
        segs += [(x0, y0, x1, y0), (x1, y0, x1, y1), (x1, y1, x0, y1), (x0, y1, x0, y0)]
    return np.array(segs, np.float64)


def _scan(pose, segs, n_beams, noise, rng):
    """Ranges of a 360-degree scan from pose (x, y, theta), the lidar at the body origin; float64."""
    ang = pose[2] + np.linspace(-math.pi, math.pi, n_beams, endpoint=False)
    d = np.stack([np.cos(ang), np.sin(ang)], 1)                        # [B, 2]
    p0, e = segs[:, :2], segs[:, 2:] - segs[:, :2]                     # [S, 2]
    w = p0[None, :, :] - np.asarray(pose[:2])[None, None, :]           # [1, S, 2]
    den = d[:, None, 0] * e[None, :, 1] - d[:, None, 1] * e[None, :, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (w[..., 0] * e[None, :, 1] - w[..., 1] * e[None, :, 0]) / den
        u = (w[..., 0] * d[:, None, 1] - w[..., 1] * d[:, None, 0]) / den
    t = np.where((np.abs(den) > 1e-12) & (t > 0) & (u >= 0) & (u <= 1), t, np.inf)
    r = t.min(1) + rng.normal(0, noise, n_beams)
    a = np.linspace(-math.pi, math.pi, n_beams, endpoint=False)
    return np.stack([r * np.cos(a), r * np.sin(a)], 1).astype(f32)   # the cloud in the body frame


class Room:
    """Two scans of one room.  Node 0 (target) at POSE_T, node 1 (source) at POSE_S in the world;
    `truth` is the source's pose in the target's frame, `est` the node estimates a caller would hold
    (the target at its truth, the source off by OFFSET in the target's frame)."""
    POSE_T = (4.0, 3.0, 0.2)
    POSE_S = (5.1, 4.2, 0.55)
    OFFSET = (-1.3, 1.2, -0.16)
    N_BEAMS = 360

    def __init__(self):
        rng = np.random.default_rng(20091)
        segs = _segments()
        self.clouds = [_scan(self.POSE_T, segs, self.N_BEAMS, 0.01, rng), _scan(self.POSE_S, segs, self.N_BEAMS, 0.01, rng)]
        ct, st = math.cos(self.POSE_T[2]), math.sin(self.POSE_T[2])
        dx, dy = self.POSE_S[0] - self.POSE_T[0], self.POSE_S[1] - self.POSE_T[1]
        self.truth = (ct * dx + st * dy, -st * dx + ct * dy, self.POSE_S[2] - self.POSE_T[2])
        self.off = tuple(t + o for t, o in zip(self.truth, self.OFFSET))
        # node estimates in the target's own frame: the target at the origin
        self.est_true = np.array([[0, 0, 0], self.truth], f32)
        self.est = np.array([[0, 0, 0], self.off], f32)
        self.pts = np.ascontiguousarray(np.concatenate(self.clouds), f32)
        self.offsets = np.array([0, self.N_BEAMS, 2 * self.N_BEAMS], np.int64)

    def error(self, pose):
        """(metres, radians) between a relative pose (x, y, theta) and the truth."""
        dth = pose[2] - self.truth[2]
        return (math.hypot(pose[0] - self.truth[0], pose[1] - self.truth[1]),
                abs(math.atan2(math.sin(dth), math.cos(dth))))


_ROOM = None


def room() -> Room:
    global _ROOM
    if _ROOM is None:
        _ROOM = Room()
    return _ROOM
