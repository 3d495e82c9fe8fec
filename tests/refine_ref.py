"""Numpy restatement of dpg_fmap_refine (the contract above dpg_refine_params in include/dpg_slam_c.h),
sharing no code with the kernel: the evaluation of a state on the interpolated field, the lane-strided
sums and their fold, the damped step, the loop with its best-iterate rule, the 200-byte record with its
covariance, and the trace.  Every float64 operation of numpy is one IEEE rounding, and a product and a
sum are two calls, so the expressions below round as the contract's do.  theta comes from the
library's dpg_refine_angle (one libm call, not repeated here), as loc_ref takes dpg_csm_lut."""
import numpy as np

from dpgslam import _abi
from dpgslam._abi import lib

f32, f64 = np.float32, np.float64
LANES, GROUP, NS, COLS = 256, 64, 11, 16
LIM = f64(2.0 ** 29)
EPS = f64(1e-12)


def params(**kw):
    p = _abi.default_refine_params()
    for k, v in kw.items():
        setattr(p, "lambda_" if k == "lambda" else k, v)
    return p


def start_of(pose):
    """dpg_refine_start's rule in numpy (the library's own cos and sin are compared with it in the tests)."""
    x, y, th = (f32(v) for v in pose)
    return np.array([x, y, th, f32(np.cos(f64(th))), f32(np.sin(f64(th)))], f32)


def starts_of(recs):
    """[B, 5] starts of track records: pose and rot."""
    recs = np.atleast_1d(recs)
    return np.concatenate([recs["pose"].reshape(-1, 3), recs["rot"].reshape(-1, 2)], 1).astype(f32)


def _field(F, box):
    x0, y0, w, h = (int(b) for b in box)
    return (np.zeros((0, 0), np.uint8) if w * h == 0 else np.asarray(F, np.uint8).reshape(h, w)), x0, y0, w, h


def _lookup(F, w, h, ix, iy):
    ok = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
    out = np.zeros(ix.shape, f64)
    if ok.any():
        out[ok] = F[iy[ok], ix[ok]].astype(f64)
    return out


def terms(F, box, ires, cloud, state):
    """Per point: used [n] and the eleven products [n, 11] (zeros where the point is not used)."""
    F, x0, y0, w, h = _field(F, box)
    tu, tv, c, s = (f64(v) for v in state)
    pts = np.asarray(cloud, f32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        x, y = pts[:, 0], pts[:, 1]
        px, py = x.astype(f64) * ires, y.astype(f64) * ires
        rx = (c * px) - (s * py)
        ry = (s * px) + (c * py)
        u, v = rx + tu, ry + tv
        used = np.isfinite(x) & np.isfinite(y) & (np.abs(u) < LIM) & (np.abs(v) < LIM)
        u, v, rx, ry = (np.where(used, a, 0.0) for a in (u, v, rx, ry))
    flu, flv = np.floor(u), np.floor(v)
    iu, iv = flu.astype(np.int64), flv.astype(np.int64)
    fu, fv = u - flu, v - flv
    au, av = 1.0 - fu, 1.0 - fv
    F00, F10 = _lookup(F, w, h, iu, iv), _lookup(F, w, h, iu + 1, iv)
    F01, F11 = _lookup(F, w, h, iu, iv + 1), _lookup(F, w, h, iu + 1, iv + 1)
    M = (av * ((au * F00) + (fu * F10))) + (fv * ((au * F01) + (fu * F11)))
    gu = (av * (F10 - F00)) + (fv * (F11 - F01))
    gv = (au * (F01 - F00)) + (fu * (F11 - F10))
    r = 255.0 - M
    jt = (gv * rx) - (gu * ry)
    T = np.stack([gu * gu, gu * gv, gu * jt, gv * gv, gv * jt, jt * jt, gu * r, gv * r, jt * r, r * r, r], 1)
    T[~used] = 0.0       # a sum never holds -0.0 (it starts from +0.0), so adding +0.0 is adding nothing
    return used, T


def sums(used, T):
    """(S [11], n_used) in the contract's order: lane t adds its points t, t + 256, ... in ascending order
    from +0.0; within each group of 64 lanes p[l] += p[l + stride] for stride 32 .. 1; (W0 + W1) + (W2 + W3)."""
    n = len(T)
    rows = -(-n // LANES)
    pad = np.zeros((rows * LANES, NS), f64)
    pad[:n] = T
    pad = pad.reshape(rows, LANES, NS)
    p = np.zeros((LANES, NS), f64)
    for k in range(rows):
        p = p + pad[k]
    W = []
    for g in range(LANES // GROUP):
        q = p[g * GROUP:(g + 1) * GROUP].copy()
        st = GROUP // 2
        while st:
            q[:st] = q[:st] + q[st:2 * st]
            st //= 2
        W.append(q[0])
    return (W[0] + W[1]) + (W[2] + W[3]), int(used.sum())


def solve(H, lam, b):
    """z of the step's expressions, or None for a failed pivot."""
    H00, H01, H02, H11, H12, H22 = (f64(v) for v in H)
    b0, b1, b2 = (f64(v) for v in b)
    lam = f64(lam)
    with np.errstate(all="ignore"):
        D1 = H11 + (lam * H11)
        D2 = H22 + (lam * H22)
        d0 = H00 + (lam * H00)
        if not d0 > 0:
            return None
        l10, l20 = H01 / d0, H02 / d0
        d1 = D1 - (l10 * H01)
        if not d1 > EPS * D1:
            return None
        e12 = H12 - (l20 * H01)
        l21 = e12 / d1
        d2 = (D2 - (l20 * H02)) - (l21 * e12)
        if not d2 > EPS * D2:
            return None
        y0 = b0
        y1 = b1 - (l10 * y0)
        y2 = (b2 - (l20 * y0)) - (l21 * y1)
        z2 = y2 / d2
        z1 = (y1 / d1) - (l21 * z2)
        z0 = ((y0 / d0) - (l10 * z1)) - (l20 * z2)
    return z0, z1, z2


def _clamp(z, m):
    return m if z > m else (-m if z < -m else z)


def step(S, state, p):
    """(status or None, next state)."""
    z = solve(S[:6], p.lambda_, S[6:9])
    if z is None or not all(np.isfinite(v) for v in z):
        return _abi.DPG_REFINE_DEGENERATE, state
    mc, ma = f64(p.max_step_cells), f64(p.max_step_angle)
    du, dv, dt = _clamp(z[0], mc), _clamp(z[1], mc), _clamp(z[2], ma)
    if abs(du) < f64(p.tol_cells) and abs(dv) < f64(p.tol_cells) and abs(dt) < f64(p.tol_angle):
        return _abi.DPG_REFINE_CONVERGED, state
    tu, tv, c, s = state
    a = dt * f64(0.5)
    q = a * a
    den = f64(1.0) + q
    cd = (f64(1.0) - q) / den
    sd = (a + a) / den
    return None, (tu + du, tv + dv, (c * cd) - (s * sd), (s * cd) + (c * sd))


def start_state(box, res, start):
    ires = f64(1.0) / f64(res)
    st = np.asarray(start, f32).reshape(5)
    tu = (f64(st[0]) * ires) - f64(int(box[0]))
    tv = (f64(st[1]) * ires) - f64(int(box[1]))
    return ires, (tu, tv, f64(st[3]), f64(st[4]))


def record(box, res, status, n_evals, best):
    """The REFINE_RESULT_DTYPE record of best = (k, state, S, n_used, cost_start)."""
    k, state, S, n_used, cost_start = best
    tu, tv, c, s = state
    res = f64(res)
    r = np.zeros((), _abi.REFINE_RESULT_DTYPE)
    r["pose"] = [f32((tu + f64(int(box[0]))) * res), f32((tv + f64(int(box[1]))) * res), f32(lib().dpg_refine_angle(float(c), float(s)))]
    r["rot"] = [f32(c), f32(s)]
    r["status"], r["n_evals"], r["best_eval"], r["n_used"] = status, n_evals, k, n_used
    r["tu"], r["tv"], r["c"], r["s"] = tu, tv, c, s
    r["cost"], r["cost_start"], r["sum_r"] = S[9], cost_start, S[10]
    r["hess"] = S[:6]
    s2 = S[9] / f64(max(n_used - 3, 1))
    cols = [solve(S[:6], 0.0, e) for e in np.eye(3)]
    if all(z is not None for z in cols):
        rr = res * res
        cov = np.array([(s2 * cols[0][0]) * rr, (s2 * cols[1][0]) * rr, (s2 * cols[2][0]) * res,
                        (s2 * cols[1][1]) * rr, (s2 * cols[2][1]) * res, s2 * cols[2][2]], f64)
        if np.isfinite(cov).all():
            r["cov"], r["cov_ok"] = cov, 1
    return r


def refine_one(F, box, res, cloud, start, p):
    """(record, trace [max_iters + 1, 16]) of one scan."""
    ires, state = start_state(box, res, start)
    K = int(p.max_iters)
    trace = np.zeros((K + 1, COLS), f64)
    best = None
    for k in range(K + 1):
        used, T = terms(F, box, ires, cloud, state)
        S, n_used = sums(used, T)
        trace[k, :4], trace[k, 4:15], trace[k, 15] = state, S, n_used
        if k == 0 or S[9] < best[2][9]:
            best = (k, state, S, n_used, S[9] if k == 0 else best[4])
        if k == 0 and n_used == 0:
            status = _abi.DPG_REFINE_NO_POINTS
        elif k == K:
            status = _abi.DPG_REFINE_MAX_ITERS
        else:
            status, state = step(S, state, p)
        if status is not None:
            return record(box, res, status, k + 1, best), trace


def refine(F, box, res, clouds, starts, p):
    """(records [B], trace [B, max_iters + 1, 16]) of a batch, scan by scan."""
    out = np.zeros(len(clouds), _abi.REFINE_RESULT_DTYPE)
    tr = np.zeros((len(clouds), int(p.max_iters) + 1, COLS), f64)
    for b, (c, s) in enumerate(zip(clouds, starts)):
        out[b], tr[b] = refine_one(F, box, res, c, s, p)
    return out, tr


def pose_error(rec, truth):
    """(metres, radians) of a record's pose from a true pose."""
    import math
    return (math.hypot(float(rec["pose"][0]) - truth[0], float(rec["pose"][1]) - truth[1]),
            abs(math.remainder(float(rec["pose"][2]) - truth[2], 2 * math.pi)))
