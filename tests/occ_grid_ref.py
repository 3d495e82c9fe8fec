"""numpy restatement of the occupancy grid (dpg_occupancy_grid, semantics in include/dpg_slam_c.h),
sharing no code with the kernel.  It takes the geometry the device reports (lidar positions and beam
end points of dpg_dpg_beam_geometry), so it repeats no libm call, and restates everything after it:
which beams are included, the float32 t chain of the free samples, the cell keys (C round, halves
away from zero), the hit / miss counting rule and the occupancy byte.  The counters are sparse
(unbounded by any box): a caller checks that every marked cell lies inside the box it was given."""
import numpy as np

L_REMOVED, L_MAX_RANGE = 2, 4
f32 = np.float32


def c_round(q):
    """C round() on float64: halves away from zero (np.round is half-to-even)."""
    q = np.asarray(q, np.float64)
    return np.sign(q) * np.floor(np.abs(q) + 0.5)


def cell_key(v, res):
    """round((double)v / res) of float32 coordinates."""
    return c_round(np.asarray(v, f32).astype(np.float64) / float(res)).astype(np.int64)


def beam_sectors(offsets, num_sectors):
    """Sector of every beam as dpg_dpg_create numbers them: (uint8)((float)i / per_sector)."""
    out = np.zeros(int(offsets[-1]), np.uint8)
    for v in range(len(offsets) - 1):
        nb = int(offsets[v + 1] - offsets[v])
        per_sector = f32(nb) / f32(num_sectors)
        out[offsets[v]:offsets[v + 1]] = (np.arange(nb, dtype=f32) / per_sector).astype(np.uint8)
    return out


def included_beams(offsets, labels, sector_active, node_active, num_sectors):
    """Mask [B]: the beam's node is active and its sector is active."""
    offsets = np.asarray(offsets, np.int64)
    node_of = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    sec = beam_sectors(offsets, num_sectors)
    return (np.asarray(node_active)[node_of] != 0) & (((np.asarray(sector_active)[node_of].astype(np.int64) >> sec) & 1) != 0)


def _count(kx, ky):
    """Sparse counters {(kx, ky): n} of a list of keys."""
    if not len(kx):
        return {}
    k = np.stack([np.concatenate(kx), np.concatenate(ky)], 1)
    u, c = np.unique(k, axis=0, return_counts=True)
    return {(int(a), int(b)): int(n) for (a, b), n in zip(u, c)}


def grid_counts(lidar_xy, end_xy, ranges, offsets, labels, sector_active, node_active, num_sectors, res):
    """(hits, misses, n_samples): sparse counters {(kx, ky): n} over the nodes of `lidar_xy`, and the
    number of free samples marched (before the hit-cell rule)."""
    offsets = np.asarray(offsets, np.int64)[:len(lidar_xy) + 1]
    B = int(offsets[-1])
    labels = np.asarray(labels, np.uint8)[:B]
    ranges = np.asarray(ranges, f32).reshape(-1)[:B]
    end = np.asarray(end_xy, f32).reshape(-1, 2)[:B]
    node_of = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    inc_mask = included_beams(offsets, labels, sector_active[:len(lidar_xy)], node_active[:len(lidar_xy)], num_sectors)
    idx = np.nonzero(inc_mask)[0]
    if not len(idx):
        return {}, {}, 0
    f = np.asarray(lidar_xy, f32)[node_of[idx]]
    m = end[idx]
    fx, fy, mx, my = f[:, 0].copy(), f[:, 1].copy(), m[:, 0].copy(), m[:, 1].copy()
    is_hit = (labels[idx] != L_MAX_RANGE) & (labels[idx] != L_REMOVED)
    ex, ey = cell_key(mx, res), cell_key(my, res)
    hits = _count([ex[is_hit]], [ey[is_hit]])
    nbins = c_round(ranges[idx].astype(np.float64) / float(res)).astype(np.uint32)
    with np.errstate(divide="ignore"):
        inc = (1.0 / nbins.astype(np.float64)).astype(f32)      # nbins = 0: inf, one sample at t = 0
    t = np.zeros(len(idx), f32)
    one = f32(1)
    kxs, kys, n_samples = [], [], 0
    while True:
        alive = t.astype(np.float64) < 1.0
        if not alive.any():
            break
        ta = t[alive]
        sx = (one - ta) * fx[alive] + ta * mx[alive]            # float32, one rounding per operation
        sy = (one - ta) * fy[alive] + ta * my[alive]
        assert sx.dtype == f32 and sy.dtype == f32
        kx, ky = cell_key(sx, res), cell_key(sy, res)
        n_samples += len(kx)
        keep = ~(is_hit[alive] & (kx == ex[alive]) & (ky == ey[alive]))   # not in its own beam's hit cell
        kxs.append(kx[keep])
        kys.append(ky[keep])
        with np.errstate(invalid="ignore"):
            t = np.where(alive, t + inc, t).astype(f32)
    return hits, _count(kxs, kys), n_samples


def occupancy(hits, misses):
    """The occupancy byte from dense counters: -1 unknown, else 100 hits / n rounded half up."""
    h = np.asarray(hits, np.int64)
    n = h + np.asarray(misses, np.int64)
    return np.where(n == 0, -1, (200 * h + n) // np.maximum(2 * n, 1)).astype(np.int8)


def to_dense(sparse, x0, y0, w, h):
    """Dense int32 [h, w] of sparse counters; every marked cell must lie inside the box."""
    out = np.zeros((h, w), np.int32)
    for (kx, ky), n in sparse.items():
        assert x0 <= kx < x0 + w and y0 <= ky < y0 + h, f"cell ({kx}, {ky}) outside the box"
        out[ky - y0, kx - x0] = n
    return out


def reference_grid(store_geometry, ranges, offsets, state, num_sectors, res, box):
    """Dense (hits, misses, data, n_samples) in the box (x0, y0, w, h) from beam_geometry's output
    (lidar_xy, end_xy) and fetch()'s state (labels, sector masks, node flags)."""
    lidar, end = store_geometry
    lab, sec, act = state
    hs, ms, ns = grid_counts(lidar, end, ranges, offsets, lab, sec, act, num_sectors, res)
    H, M = to_dense(hs, *box), to_dense(ms, *box)
    return H, M, occupancy(H, M), ns
