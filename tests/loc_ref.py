"""Numpy restatement of the localisation in the active map (the contract above dpg_loc_params in
include/dpg_slam_c.h), sharing no code with the kernels: the field F from the occupancy bytes, the
pooled field P, the keys, the bound volume, the brute-force score volume, the winner with its tie
order, the record -- and the pruned search (seeds, best0, frontier, overflow), so that the two can
be compared on the CPU.  The smoothing bytes and the rotation table come from the exported host
functions (dpg_csm_lut, dpg_loc_rotations), so no libm call is repeated here; everything else is
integer or a float32 operation numpy rounds once."""
import numpy as np

from occ_grid_ref import c_round
from dpgslam import _abi, api

f32 = np.float32
LIMIT = 536870912.0   # 2^29


def keys(pts, res):
    """(kx, ky, valid) of float32 points [N, 2]: key = round((double)v / res), res a double (the grid's
    rule); a point with a non-finite coordinate or |v / res| >= 2^29 is not valid."""
    q = np.asarray(pts, f32).reshape(-1, 2).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = q / float(res)
        valid = np.isfinite(d).all(1) & (np.abs(d) < LIMIT).all(1)
    k = c_round(np.where(valid[:, None], d, 0.0)).astype(np.int64)
    return k[:, 0], k[:, 1], valid


def lut_of(p, res):
    """dpg_csm_lut's bytes for ((float)res, sigma, kernel_radius)."""
    cp = _abi.default_csm_params()
    cp.resolution, cp.sigma, cp.kernel_radius = float(f32(res)), p.sigma, p.kernel_radius
    return api.csm_lut(cp)


def field(occ, p, res):
    """F, uint8 [h, w], from the occupancy bytes int8 [h, w]."""
    occ = np.asarray(occ, np.int8)
    h, w = occ.shape
    lut, R = lut_of(p, res), int(p.kernel_radius)
    occupied = occ.astype(np.int64) >= int(p.occupied_min)
    pad = np.zeros((h + 2 * R, w + 2 * R), bool)
    pad[R:R + h, R:R + w] = occupied
    F = np.zeros((h, w), np.uint8)
    for oy in range(-R, R + 1):
        for ox in range(-R, R + 1):
            d2 = ox * ox + oy * oy
            if d2 <= R * R:   # the cell at (x + ox, y + oy) is occupied
                F = np.maximum(F, np.where(pad[R + oy:R + oy + h, R + ox:R + ox + w], lut[d2], 0).astype(np.uint8))
    return F


def pooled(F, shift):
    """P, uint8 [h + s - 1, w + s - 1]: P[y + s - 1, x + s - 1] = max F[y .. y + s - 1, x .. x + s - 1]."""
    s = 1 << shift
    h, w = F.shape
    big = np.zeros((h + 2 * (s - 1), w + 2 * (s - 1)), np.uint8)
    big[s - 1:s - 1 + h, s - 1:s - 1 + w] = F
    P = np.zeros((h + s - 1, w + s - 1), np.uint8)
    for j in range(s):
        for i in range(s):
            P = np.maximum(P, big[j:j + h + s - 1, i:i + w + s - 1])
    return P


def point_keys(cloud, rot_a, res):
    """Keys of the points at one angle: r = ((c x) - (s y), (s x) + (c y)) in float32."""
    q = np.asarray(cloud, f32).reshape(-1, 2)
    c, s = f32(rot_a[0]), f32(rot_a[1])
    x, y = q[:, 0], q[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        rx = (c * x) - (s * y)
        ry = (s * x) + (c * y)
    assert rx.dtype == f32 and ry.dtype == f32
    kx, ky, ok = keys(np.stack([rx, ry], 1), res)
    return kx[ok], ky[ok]


def guess_keys(guess, res):
    kx, ky, ok = keys(np.asarray(guess, f32).reshape(3)[None, :2], res)
    assert ok[0], "the guess has no valid key"
    return int(kx[0]), int(ky[0])


def _volume(T, x0s, y0s, nx, ny, step):
    """sum over the points of T[y0 + j step, x0 + i step], j < ny, i < nx, zero outside T: int64 [ny, nx]."""
    H, W = T.shape
    acc = np.zeros((ny, nx), np.int64)
    for x0, y0 in zip(x0s.tolist(), y0s.tolist()):
        i0, i1 = max(0, -(x0 // step)), min(nx, (W - 1 - x0) // step + 1)
        j0, j1 = max(0, -(y0 // step)), min(ny, (H - 1 - y0) // step + 1)
        if i0 < i1 and j0 < j1:
            acc[j0:j1, i0:i1] += T[y0 + j0 * step:y0 + (j1 - 1) * step + 1:step, x0 + i0 * step:x0 + (i1 - 1) * step + 1:step]
    return acc


class Problem:
    """One request: the field of `occ` in `box` = (x0, y0, w, h), a cloud, a guess and the params."""

    def __init__(self, occ, box, res, cloud, guess, p):
        self.p, self.res, self.box = p, float(res), tuple(int(b) for b in box)
        self.cloud = np.asarray(cloud, f32).reshape(-1, 2)
        self.guess = np.asarray(guess, f32).reshape(3)
        self.hx, self.hy, self.ha = int(p.half_x), int(p.half_y), int(p.half_a)
        self.shift, self.s = int(p.coarse_shift), 1 << int(p.coarse_shift)
        self.A = 2 * self.ha + 1
        self.nbx = (2 * self.hx + self.s) // self.s
        self.nby = (2 * self.hy + self.s) // self.s
        self.empty = self.box[2] * self.box[3] == 0
        self.F = np.zeros((0, 0), np.uint8) if self.empty else field(occ, p, res)
        self.P = self.F if self.empty else pooled(self.F, self.shift)
        self.rot = api.loc_rotations(self.guess[2], p)
        self.cx, self.cy = guess_keys(self.guess, res)
        self._keys = {}

    def keys_at(self, a):
        """The points' field indices at the window's first shift (-hx, -hy)."""
        if a not in self._keys:
            kx, ky = point_keys(self.cloud, self.rot[a], self.res)
            self._keys[a] = (kx + self.cx - self.hx - self.box[0], ky + self.cy - self.hy - self.box[1])
        return self._keys[a]

    def bounds(self):
        """int32 [A, nby, nbx]."""
        vol = np.zeros((self.A, self.nby, self.nbx), np.int64)
        if not self.empty:
            Pi = self.P.astype(np.int64)
            for a in range(self.A):
                ux, uy = self.keys_at(a)
                vol[a] = _volume(Pi, ux + self.s - 1, uy + self.s - 1, self.nbx, self.nby, self.s)
        assert vol.max(initial=0) < 2 ** 31
        return vol.astype(np.int32)

    def scores(self):
        """The brute-force volume, int32 [A, 2 hy + 1, 2 hx + 1]."""
        vol = np.zeros((self.A, 2 * self.hy + 1, 2 * self.hx + 1), np.int64)
        if not self.empty:
            Fi = self.F.astype(np.int64)
            for a in range(self.A):
                ux, uy = self.keys_at(a)
                vol[a] = _volume(Fi, ux, uy, 2 * self.hx + 1, 2 * self.hy + 1, 1)
        assert vol.max(initial=0) < 2 ** 31
        return vol.astype(np.int32)

    def block_scores(self, a, bx, by):
        """The exact scores of one block's in-window candidates: (scores [ny, nx], dx0, dy0)."""
        dx0, dy0 = -self.hx + bx * self.s, -self.hy + by * self.s
        nx, ny = min(self.s, self.hx - dx0 + 1), min(self.s, self.hy - dy0 + 1)
        if self.empty:
            return np.zeros((ny, nx), np.int64), dx0, dy0
        ux, uy = self.keys_at(a)
        h, w = self.F.shape
        Fz = self._Fz()
        X = ux[:, None] + (bx * self.s + np.arange(nx))[None, :]
        Y = uy[:, None] + (by * self.s + np.arange(ny))[None, :]
        X = np.where((X >= 0) & (X < w), X, w)
        Y = np.where((Y >= 0) & (Y < h), Y, h)
        return Fz[Y[:, :, None], X[:, None, :]].sum(0), dx0, dy0

    def _Fz(self):
        if not hasattr(self, "_fz"):
            h, w = self.F.shape
            self._fz = np.zeros((h + 1, w + 1), np.int64)   # a zero row and column: clipped indices land there
            self._fz[:h, :w] = self.F
        return self._fz

    # ---- orders
    def cand_key(self, score, a, dx, dy):
        """Sort key, smallest first = the winner."""
        return (-int(score), abs(a - self.ha), dx * dx + dy * dy, a, dy, dx)

    def winner_of(self, vol):
        a, iy, ix = np.nonzero(vol == vol.max())
        best = min(self.cand_key(vol[q, y, x], int(q), int(x) - self.hx, int(y) - self.hy) for q, y, x in zip(a, iy, ix))
        return -best[0], best[3], best[5], best[4]   # score, a, dx, dy

    def seeds(self, bvol):
        """Per angle (bound, by, bx): the highest bound, then the block nearest the centre, then by, bx."""
        out = []
        for a in range(self.A):
            by, bx = np.nonzero(bvol[a] == bvol[a].max())
            mx = 2 * (bx.astype(np.int64) * self.s - self.hx) + self.s - 1
            my = 2 * (by.astype(np.int64) * self.s - self.hy) + self.s - 1
            _, y, x = min(zip((mx * mx + my * my).tolist(), by.tolist(), bx.tolist()))
            out.append((int(bvol[a, y, x]), y, x))
        return out

    # ---- records
    def record(self, score, a, dx, dy, status, score_at_guess, n_frontier, n_refined):
        r = np.zeros((), _abi.LOC_RESULT_DTYPE)
        res = np.float64(self.res)
        ang = np.float64(self.guess[2]) + np.float64(a - self.ha) * np.float64(f32(self.p.angle_step))
        r["pose"] = [f32(np.float64(self.cx + dx) * res), f32(np.float64(self.cy + dy) * res), f32(ang)]
        r["rot"] = self.rot[a]
        r["score"], r["score_at_guess"], r["n_pts"] = score, score_at_guess, len(self.cloud)
        r["best_a"], r["best_dx"], r["best_dy"] = a, dx, dy
        r["status"], r["n_seeds"], r["box"] = status, self.A, self.box
        r["n_blocks"], r["n_frontier"], r["n_refined_candidates"] = self.A * self.nbx * self.nby, n_frontier, n_refined
        return r

    def score_at_guess(self):
        bx, by = self.hx // self.s, self.hy // self.s
        sc, dx0, dy0 = self.block_scores(self.ha, bx, by)
        return int(sc[-dy0, -dx0])

    def search(self, bvol=None):
        """The pruned search's record (timings zero)."""
        if self.empty:
            return self.record(0, self.ha, 0, 0, _abi.DPG_LOC_NO_OVERLAP, 0, 0, 0)
        bvol = self.bounds() if bvol is None else bvol
        seeds = self.seeds(bvol)

        def best_of(blocks):
            best, n = None, 0
            for a, by, bx in blocks:
                sc, dx0, dy0 = self.block_scores(a, bx, by)
                n += sc.size
                for j, i in zip(*np.nonzero(sc == sc.max())):
                    k = self.cand_key(sc[j, i], a, dx0 + int(i), dy0 + int(j))
                    best = k if best is None or k < best else best
            return best, n

        k0, n0 = best_of([(a, y, x) for a, (_, y, x) in enumerate(seeds)])
        best0 = -k0[0]
        fa, fy, fx = np.nonzero(bvol >= best0)
        cap = min(int(self.p.max_refine_blocks), bvol.size)
        overflow = len(fa) > cap
        k, n = k0, n0
        if not overflow:
            k1, n1 = best_of(zip(fa.tolist(), fy.tolist(), fx.tolist()))
            k, n = min(k0, k1), n0 + n1
        score = -k[0]
        if score == 0 and (max(b for b, _, _ in seeds) == 0 or not overflow):
            status = _abi.DPG_LOC_NO_OVERLAP
        else:
            status = _abi.DPG_LOC_UNPROVEN if overflow else _abi.DPG_LOC_OK
        return self.record(score, k[3], k[5], k[4], status, self.score_at_guess(), len(fa), n)

    def brute(self, vol=None):
        """(score, a, dx, dy) of the exhaustive search."""
        return self.winner_of(self.scores() if vol is None else vol)


def same_record(a, b):
    """Two records agree in every field but the timings."""
    return all(np.array_equal(a[n], b[n]) for n in _abi.LOC_RESULT_EXACT)
