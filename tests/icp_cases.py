"""Adversarial clouds for the batched ICP kernels (a helper module like graphs.py, not a test).

Every generator is deterministic (fixed seeds) and returns float32 points.  A case is what
Context.upload_scans / icp_batch and oracle.icp_batch take: (pts, offsets, est, edges, parameter
overrides), plus its name and the downsample ratio the clouds are uploaded at (1 unless stated).
An edge is (target node, source node).  Clouds are kept at the smallest size that still reaches the
branch the case is for; the groups are

  sizes   rooms of n points on and next to every switch of the angular kernel's forms
  mixed   unequal pairs in one batch (a 3-point cloud under the form a 4097-point one selects)
  empty   nodes of no points
  ties    lattices: exact distance ties and duplicated points (the lowest index must win)
  angles  points on the octant seams of the pseudo-angle, the origin, -0.0, collinear rays
  range   clouds within 10 cm of the origin and 100 m out
  params  correspondence distance, reciprocity, min_number_correspondences, bad guesses
  ratio   the device downsample's ceil at ratio 3
"""
from dataclasses import dataclass, field

import numpy as np

SIZES_SMALL = (1, 2, 3, 4, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096)
SIZES_16 = (4097, 8191, 8192)      # 16 points per lane, source records in global scratch
SIZES_32 = (8193, 16383, 16384)    # 32 points per lane, both record sets there
MIXED_PAIRS = ((3, 4096), (4096, 3), (1, 100), (100, 1), (65, 513), (5, 4097), (4097, 5))   # (source, target)
KD_GRID_MAX = 4096                 # the k-d tree and grid variants take no larger cloud
TRACE_ITERS = 16


@dataclass
class Case:
    name: str
    pts: np.ndarray        # float32 [P, 2], the nodes' full clouds one after the other
    offsets: np.ndarray    # int64 [V + 1]
    est: np.ndarray        # float32 [V, 3]
    edges: np.ndarray      # int32 [E, 2] = (target, source)
    overrides: dict = field(default_factory=dict)   # dpg_icp_params fields that differ from the defaults
    ratio: int = 1
    expect_fail: bool = False   # built to end DPG_ICP_TOO_FEW_CORR on every edge

    def __iter__(self):
        return iter((self.pts, self.offsets, self.est, self.edges, self.overrides))

    @property
    def group(self):
        return self.name.split("/")[0]

    def params(self):
        from dpgslam import _abi
        p = _abi.default_icp_params()
        p.downsample_icp_points_ratio = self.ratio
        for k, v in self.overrides.items():
            assert hasattr(p, k), k
            setattr(p, k, v)
        return p

    def cloud(self, v):
        return self.pts[self.offsets[v]:self.offsets[v + 1]]

    def max_points(self):
        """The largest downsampled cloud: what selects the kernel form."""
        n = np.diff(self.offsets)
        return int(((n + self.ratio - 1) // self.ratio).max())


def _case(name, clouds, est, edges, overrides=None, ratio=1, expect_fail=False):
    clouds = [np.asarray(c, np.float32).reshape(-1, 2) for c in clouds]
    pts = np.concatenate(clouds).astype(np.float32) if clouds else np.zeros((0, 2), np.float32)
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    return Case(name, pts, offsets, np.asarray(est, np.float32).reshape(-1, 3),
                np.asarray(edges, np.int32).reshape(-1, 2), dict(overrides or {}), ratio, expect_fail)


# ------------------------------------------------------------------------------ clouds
ROOM_HALF = (3.0, 2.0)              # a 6 m x 4 m room around the origin
TRUE_POSES = np.array([[0.0, 0.0, 0.0], [0.12, -0.08, 0.03]])
PERTURB = np.array([0.05, -0.04, 0.02])   # the source estimate's error: the work the alignment has to do


def room_cloud(n, pose, seed, noise=0.005, scale=1.0, beams=None):
    """n beams, evenly spaced over the full turn in angle order, cast from `pose` (inside the room)
    to the walls of the room; points in the frame of the pose, times `scale`.  beams: a slice of the
    n beams to keep (a partial view)."""
    rng = np.random.default_rng(seed)
    a = -np.pi + 2.0 * np.pi * (np.arange(n) + 0.5) / max(n, 1)
    x, y, th = pose
    dx, dy = np.cos(a + th), np.sin(a + th)
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = np.where(dx > 0, (ROOM_HALF[0] - x) / dx, np.where(dx < 0, (-ROOM_HALF[0] - x) / dx, np.inf))
        ty = np.where(dy > 0, (ROOM_HALF[1] - y) / dy, np.where(dy < 0, (-ROOM_HALF[1] - y) / dy, np.inf))
    r = np.minimum(tx, ty) + rng.normal(0.0, noise, n)
    p = np.stack([r * np.cos(a), r * np.sin(a)], 1) * scale
    if beams is not None:
        p = p[beams]
    return p.astype(np.float32)


def room_pair(n_src, n_tgt, seed, scale=1.0, perturb=PERTURB, noise=0.005, src_beams=None):
    """(clouds [target, source], est): node 0 the target at the origin, node 1 the source a small
    rigid offset away (times `scale`, like the room), its estimate off by `perturb` (as given)."""
    tgt = room_cloud(n_tgt, TRUE_POSES[0], seed, noise, scale)
    src = room_cloud(n_src, TRUE_POSES[1], seed + 1000, noise, scale, src_beams)
    est = TRUE_POSES.copy()
    est[:, :2] *= scale
    est[1] += perturb
    return [tgt, src], est.astype(np.float32)


BOTH = ((0, 1), (1, 0))


def lattice(n=16, h=0.25):
    """n x n points at spacing h, x fastest, centred so that point (n/2, n/2) is the origin: every
    coordinate is a multiple of h (exact in float), the cloud covers every octant seam."""
    k = (np.arange(n) - n // 2) * h
    return np.stack([np.tile(k, n), np.repeat(k, n)], 1).astype(np.float32)


def ray(angle_index, n=400, r0=0.5, r1=20.0, jitter=0.0):
    """n points from r0 to r1 along +x (0), -x (1) or the +x+y diagonal (2), exactly on the seam;
    jitter: alternate points that far to either side of it."""
    r = np.linspace(r0, r1, n).astype(np.float32)
    z = np.zeros_like(r)
    side = (jitter * (1 - 2 * (np.arange(n) % 2))).astype(np.float32)
    if angle_index == 0:
        p = np.stack([r, z + side], 1)
    elif angle_index == 1:
        p = np.stack([-r, z + side], 1)
    else:
        d = (r * np.float32(np.sqrt(0.5))).astype(np.float32)
        p = np.stack([d - side, d + side], 1)
    return p.astype(np.float32)


def seam_points():
    """Points exactly on +-x, +-y and the four diagonals at eight radii, the origin, and their
    twins written with -0.0 coordinates (equal as numbers: exact duplicates, at other indices)."""
    out = [(0.0, 0.0)]
    for k in range(1, 9):
        r = 0.5 * k
        d = r * 0.75   # exact in float, and |x| == |y| exactly
        out += [(r, 0.0), (d, d), (0.0, r), (-d, d), (-r, 0.0), (-d, -d), (0.0, -r), (d, -d)]
    out += [(-0.0, -0.0), (0.75, -0.0), (-0.0, 0.75), (-0.75, -0.0), (-0.0, -0.75), (-0.0, 0.0), (0.0, -0.0),
            (1.0, -0.0), (-0.0, 1.0)]
    return np.array(out, np.float32)


# ------------------------------------------------------------------------------ groups
def sizes_cases():
    out = []
    for n in SIZES_SMALL + SIZES_16 + SIZES_32:
        # above 4096 points the room grows with the cloud, so that the point spacing (and with it the
        # oracle's work per query) stays that of a 1024-point room
        clouds, est = room_pair(n, n, seed=n, scale=n / 1024.0 if n > KD_GRID_MAX else 1.0)
        out.append(_case(f"sizes/n{n}", clouds, est, BOTH))
    # every small size in one batch: the small clouds under the 8-points-per-lane form
    clouds, est, edges = [], [], []
    for n in SIZES_SMALL:
        c, e = room_pair(n, n, seed=n)
        edges.append((len(clouds), len(clouds) + 1))
        clouds += c
        est += list(e)
    out.append(_case("sizes/all", clouds, est, edges))
    return out


def _mixed(name, pairs):
    clouds, est, edges = [], [], []
    for k, (ns, nt) in enumerate(pairs):
        c, e = room_pair(ns, nt, seed=50 + k)
        edges.append((len(clouds), len(clouds) + 1))
        clouds += c
        est += list(e)
    return _case(name, clouds, est, edges)


def mixed_cases():
    """mixed/all is the batch of every pair (angular only: it holds 4097-point clouds);
    mixed/le4096 the pairs the other two variants take as well; mixed/src_larger one direction only."""
    return [_mixed("mixed/all", MIXED_PAIRS),
            _mixed("mixed/le4096", [p for p in MIXED_PAIRS if max(p) <= KD_GRID_MAX]),
            # every source larger than every target: the batch's largest cloud is not a target
            _mixed("mixed/src_larger", [(4096, 3), (100, 1), (513, 65)])]


def empty_cases():
    """Nodes 0, 1: no points; node 2: 5 points; nodes 3, 4: an ordinary 100-point pair."""
    c5 = room_cloud(5, TRUE_POSES[1], 7)
    pair, est = room_pair(100, 100, seed=8)
    z = np.zeros((0, 2), np.float32)
    est_all = np.concatenate([[[0, 0, 0], [0.1, 0.05, 0.01], [0.02, -0.03, 0.02]], est]).astype(np.float32)
    edges = [(0, 1), (1, 0), (0, 2), (2, 0), (3, 4), (4, 3)]
    return [_case("empty/batch", [z, z, c5] + pair, est_all, edges)]


def ties_cases():
    L = lattice()
    z = np.zeros((2, 3), np.float32)
    h = np.float32(0.125)
    c, s = np.float32(np.cos(0.02)), np.float32(np.sin(0.02))
    rot = np.stack([c * L[:, 0] - s * L[:, 1], s * L[:, 0] + c * L[:, 1]], 1).astype(np.float32)
    dup = np.concatenate([L, L[::-1]])
    shift = np.array([0.05, 0.03], np.float32)
    return [
        _case("ties/half_x", [L, L + np.array([h, 0], np.float32)], z, BOTH),
        _case("ties/half_diag", [L, L + np.array([h, h], np.float32)], z, [(0, 1)], expect_fail=True),
        _case("ties/dup_reversed", [dup, dup + shift], z, BOTH),
        _case("ties/rotated", [L, rot], z, BOTH),
    ]


def angles_cases():
    S = seam_points()
    est = np.array([[0, 0, 0], [0.03, -0.02, 0.01]], np.float32)
    out = [_case("angles/seams", [S, S], est, BOTH)]
    for k, name in enumerate(("ray_px", "ray_nx", "ray_diag")):
        out.append(_case(f"angles/{name}", [ray(k), ray(k, jitter=0.002)], est, BOTH))
    return out


def range_cases():
    out = []
    for r in (0.6, 0.05):
        clouds, est = room_pair(300, 300, seed=21, scale=0.02, perturb=PERTURB * (0.02, 0.02, 1.0))
        out.append(_case(f"range/near_r{r}", clouds, est, BOTH, {"icp_max_correspondence_distance": r}))
    clouds, est = room_pair(3000, 3000, seed=22, scale=30.0, perturb=PERTURB * (4.0, 4.0, 4.0 / 30.0), noise=0.0005)
    out.append(_case("range/far", clouds, est, BOTH))
    return out


PARAMS_PERTURB = np.array([0.006, -0.005, 0.001])   # inside the smallest radius tried


def params_cases():
    out = []
    clouds, est = room_pair(700, 700, seed=31, perturb=PARAMS_PERTURB, noise=0.001)
    for r in (0.02, 0.1, 2.0, 10.0):
        out.append(_case(f"params/r{r}", clouds, est, BOTH, {"icp_max_correspondence_distance": r}))
    out.append(_case("params/no_reciprocal", clouds, est, BOTH, {"icp_use_reciprocal_correspondences": 0}))
    for m in (1, 2):
        out.append(_case(f"params/min_corr{m}", clouds, est, BOTH, {"min_number_correspondences": m}))
    c, e = room_pair(1, 100, seed=50 + MIXED_PAIRS.index((1, 100)))   # the (1, 100) pair of the mixed group
    out.append(_case("params/one_point_min_corr1", c, e, [(0, 1)], {"min_number_correspondences": 1}))
    c, e = room_pair(200, 200, seed=32)
    c[1] = c[1] + np.array([50.0, 0.0], np.float32)
    out.append(_case("params/disjoint", c, e, BOTH, expect_fail=True))
    c, e = room_pair(700, 700, seed=33)
    e = e.copy()
    e[1, 2] += 3.0
    out.append(_case("params/guess_3rad", c, e, BOTH))
    c, e = room_pair(900, 700, seed=34, src_beams=slice(300, 600))
    out.append(_case("params/partial_overlap", c, e, BOTH))
    return out


RATIO_FULL = (1, 2, 3, 4, 7, 1025)


def ratio_cases():
    """Full clouds of 1 .. 1025 points uploaded at ratio 3: ceil(n / 3) = 1, 1, 1, 2, 3, 342."""
    clouds, est, edges = [], [], []
    for n in RATIO_FULL:
        c, e = room_pair(n, n, seed=60 + n)
        edges += [(len(clouds), len(clouds) + 1), (len(clouds) + 1, len(clouds))]
        clouds += c
        est += list(e)
    edges += [(8, 11), (11, 8)]   # 7 points against 1025
    return [_case("ratio/r3", clouds, est, edges, ratio=3)]


GROUPS = {"sizes": sizes_cases, "mixed": mixed_cases, "empty": empty_cases, "ties": ties_cases,
          "angles": angles_cases, "range": range_cases, "params": params_cases, "ratio": ratio_cases}

_CACHE = {}


def cases(group):
    if group not in _CACHE:
        _CACHE[group] = GROUPS[group]()
    return _CACHE[group]


def case(name):
    for c in cases(name.split("/")[0]):
        if c.name == name:
            return c
    raise KeyError(name)


def all_names(groups=None):
    return [c.name for g in (groups or GROUPS) for c in cases(g)]
