"""Numpy restatement of dpg_fmap_track (the contract above dpg_track_params in include/dpg_slam_c.h),
sharing no code with the kernels.  A tracked scan's record is the EXHAUSTIVE search of its window on
the map's field: the volume and the winner are loc_ref.Problem.scores() / .brute() for the same
half_x, half_y, half_a, angle_step and guess at coarse_shift 0; this file adds the problem over a
given field (a frozen map holds F, not occupancy bytes) and the 48-byte record."""
import numpy as np

import loc_ref as L
from dpgslam import _abi, api

f32 = np.float32


def loc_params(tp, res=0.0, **kw):
    """The dpg_loc_params whose exhaustive search is tp's: same window and step, coarse_shift 0."""
    p = _abi.default_loc_params()
    p.resolution = float(res)
    p.half_x, p.half_y, p.half_a, p.angle_step = int(tp.half_x), int(tp.half_y), int(tp.half_a), float(tp.angle_step)
    p.coarse_shift = 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def track_params(half_x=10, half_y=10, half_a=10, angle_step=None):
    p = _abi.default_track_params()
    p.half_x, p.half_y, p.half_a = half_x, half_y, half_a
    if angle_step is not None:
        p.angle_step = angle_step
    return p


class Problem(L.Problem):
    """One scan against a field F (uint8 [h, w]) in box = (x0, y0, w, h) at `res`."""

    def __init__(self, F, box, res, cloud, guess, tp):
        p = loc_params(tp, res)
        self.p, self.res, self.box = p, float(res), tuple(int(b) for b in box)
        self.cloud = np.asarray(cloud, f32).reshape(-1, 2)
        self.guess = np.asarray(guess, f32).reshape(3)
        self.hx, self.hy, self.ha = int(p.half_x), int(p.half_y), int(p.half_a)
        self.shift, self.s = 0, 1
        self.A = 2 * self.ha + 1
        self.nbx, self.nby = 2 * self.hx + 1, 2 * self.hy + 1
        self.empty = self.box[2] * self.box[3] == 0
        self.F = np.zeros((0, 0), np.uint8) if self.empty else np.asarray(F, np.uint8).reshape(self.box[3], self.box[2])
        self.P = self.F
        self.rot = api.loc_rotations(self.guess[2], p)
        self.cx, self.cy = L.guess_keys(self.guess, res)
        self._keys = {}

    def track_record(self, vol=None):
        """The TRACK_RESULT_DTYPE record."""
        vol = self.scores() if vol is None else vol
        score, a, dx, dy = self.brute(vol)
        r = np.zeros((), _abi.TRACK_RESULT_DTYPE)
        res = np.float64(self.res)
        ang = np.float64(self.guess[2]) + np.float64(a - self.ha) * np.float64(f32(self.p.angle_step))
        r["pose"] = [f32(np.float64(self.cx + dx) * res), f32(np.float64(self.cy + dy) * res), f32(ang)]
        r["rot"] = self.rot[a]
        r["score"], r["score_at_guess"], r["n_pts"] = score, int(vol[self.ha, self.hy, self.hx]), len(self.cloud)
        r["best_a"], r["best_dx"], r["best_dy"] = a, dx, dy
        r["status"] = _abi.DPG_LOC_NO_OVERLAP if score == 0 else _abi.DPG_LOC_OK
        return r


def track(F, box, res, clouds, guesses, tp):
    """The records of a batch, scan by scan."""
    out = np.zeros(len(clouds), _abi.TRACK_RESULT_DTYPE)
    for b, (c, g) in enumerate(zip(clouds, guesses)):
        out[b] = Problem(F, box, res, c, g, tp).track_record()
    return out


def same_as_loc(t, r):
    """A track record agrees with a dpg_loc_result record in every field they share."""
    return all(np.array_equal(t[n], r[n]) for n in _abi.TRACK_RESULT_DTYPE.names)
