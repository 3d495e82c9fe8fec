"""The oracle on the adversarial clouds of icp_cases.py, before it is used as the reference of
test_icp_adversarial.py: its two searches (brute force, grid) and its two entries (per-edge
icp_align, icp_batch) agree byte for byte on every case, and the cases do what they were built for
-- the GPU test would pass vacuously on a `params` case that never iterates or a "failing" case
that converges.  Clouds above 4096 points run the grid search only (brute force at 16384^2 per
iteration is no unit test)."""
import numpy as np
import pytest

import icp_cases as C

FIELDS = ("T", "z", "converged", "iterations", "n_corr", "status", "fitness")
BRUTE_MAX = 4096
_ALIGN = {}
_BATCH = {}


def _align(src, tgt, guess, p, nn, trace=0):
    """O.icp_align, remembered by its inputs (sizes/all repeats the clouds of the sizes/nN cases)."""
    from oracle import oracle as O
    key = (src.tobytes(), tgt.tobytes(), guess.tobytes(), bytes(p), nn, trace)
    if key not in _ALIGN:
        _ALIGN[key] = O.icp_align(src, tgt, guess, p, nn, trace_iters=trace)
    return _ALIGN[key]


def _batch(c):
    from oracle import oracle as O
    if c.name not in _BATCH:
        _BATCH[c.name] = O.icp_batch(c.pts, c.offsets, c.edges, c.est, c.params(), O.NN_GRID, threads=8)[0]
    return _BATCH[c.name]


def _n_src(c, e):
    n = int(c.offsets[c.edges[e, 1] + 1] - c.offsets[c.edges[e, 1]])
    return (n + c.ratio - 1) // c.ratio


@pytest.mark.parametrize("name", C.all_names())
def test_oracle_searches_and_entries_agree(name):
    from dpgslam import _abi, api
    from oracle import oracle as O
    c = C.case(name)
    p = c.params()
    ref = _batch(c)
    for e, (t, s) in enumerate(c.edges):
        sd, td = O.downsample(c.cloud(s), c.ratio), O.downsample(c.cloud(t), c.ratio)
        assert len(sd) == _n_src(c, e)
        # the product's host downsample (what the device one is checked against through the results)
        assert api.downsample(c.cloud(s), c.ratio).tobytes() == sd.tobytes()
        g = O.icp_guess(c.est[s], c.est[t])
        rg, tg = _align(sd, td, g, p, O.NN_GRID, C.TRACE_ITERS)
        one = np.frombuffer(bytes(rg), _abi.RESULT_DTYPE)[0]
        for k in FIELDS:
            assert np.asarray(one[k]).tobytes() == np.asarray(ref[k][e]).tobytes(), f"{name} edge {e}: batch vs align, {k}"
        if max(len(sd), len(td)) <= BRUTE_MAX:
            rb, tb = _align(sd, td, g, p, O.NN_BRUTE, C.TRACE_ITERS)
            assert bytes(rb) == bytes(rg), f"{name} edge {e}: brute vs grid"
            assert tb.tobytes() == tg.tobytes(), f"{name} edge {e}: brute vs grid, correspondences"


def _ok(res):
    return (res["converged"] == 1) & (res["status"] == 0) & (res["iterations"] >= 2)


@pytest.mark.parametrize("name", [n for n in C.all_names(("sizes", "range", "params"))])
def test_cases_converge_or_fail_as_built(name):
    from dpgslam import _abi
    c = C.case(name)
    res = _batch(c)
    if c.expect_fail:
        assert np.all(res["status"] == _abi.DPG_ICP_TOO_FEW_CORR) and not res["converged"].any(), res
        return
    if c.group == "sizes":   # below 63 points a cloud may have fewer than three correspondences
        keep = np.array([_n_src(c, e) >= 63 for e in range(len(c.edges))])
        res = res[keep]
        if c.max_points() < 63:
            return
        assert len(res)
    assert np.all(_ok(res)), (name, res[["converged", "status", "iterations", "n_corr"]])


def test_failing_cases_fail_and_one_keeps_correspondences():
    from dpgslam import _abi
    built = [c for g in C.GROUPS for c in C.cases(g) if c.expect_fail]
    assert {c.name for c in built} >= {"ties/half_diag", "params/disjoint"}
    n_corr = []
    for c in built:
        res = _batch(c)
        assert np.all(res["status"] == _abi.DPG_ICP_TOO_FEW_CORR), c.name
        n_corr += list(res["n_corr"])
    assert max(n_corr) > 0 and min(n_corr) == 0   # too few of some, and none at all
    assert _batch(C.case("ties/half_diag"))["n_corr"][0] == 1


def test_ties_break_reciprocity():
    """At least one lattice case keeps fewer than half of its points: among equidistant candidates the
    lowest index wins in both directions, so most forward matches are not returned."""
    worst = min(float(res_n) / _n_src(c, e) for c in C.cases("ties")
                for e, res_n in enumerate(_batch(c)["n_corr"]))
    assert worst < 0.5
    dup = C.case("ties/dup_reversed")
    assert np.all(_batch(dup)["n_corr"] * 2 <= [_n_src(dup, e) for e in range(len(dup.edges))])


def test_no_reciprocal_keeps_every_point():
    c = C.case("params/no_reciprocal")
    res = _batch(c)
    assert list(res["n_corr"]) == [_n_src(c, e) for e in range(len(c.edges))]


def test_one_correspondence_fit_is_reached():
    """One source point at min_number_correspondences = 1: the rigid fit's h == 0 branch (identity
    rotation), two iterations."""
    res = _batch(C.case("params/one_point_min_corr1"))
    assert (res["converged"][0], res["status"][0], res["iterations"][0], res["n_corr"][0]) == (1, 0, 2, 1)


def test_empty_clouds_oracle_contract():
    """An edge with an empty cloud: TOO_FEW_CORR, no iteration, T = the guess."""
    from dpgslam import _abi
    from oracle import oracle as O
    c = C.case("empty/batch")
    res = _batch(c)
    n = np.diff(c.offsets)
    for e, (t, s) in enumerate(c.edges):
        if n[t] and n[s]:
            assert _ok(res[e:e + 1])[0]
            continue
        assert (res["converged"][e], res["status"][e], res["iterations"][e], res["n_corr"][e]) == \
            (0, _abi.DPG_ICP_TOO_FEW_CORR, 0, 0)
        assert res["T"][e].tobytes() == O.icp_guess(c.est[s], c.est[t]).tobytes()
        assert res["fitness"][e] == 0.0


def test_case_shapes():
    """The generators give what the table of the groups says: sizes, dtypes, determinism."""
    for g in C.GROUPS:
        for c in C.cases(g):
            assert c.pts.dtype == np.float32 and c.est.dtype == np.float32 and c.edges.dtype == np.int32
            assert c.offsets[-1] == len(c.pts) and np.isfinite(c.pts).all()
            again = [x for x in C.GROUPS[g]() if x.name == c.name][0]
            assert again.pts.tobytes() == c.pts.tobytes() and again.est.tobytes() == c.est.tobytes()
    for n in C.SIZES_SMALL + C.SIZES_16 + C.SIZES_32:
        assert list(np.diff(C.case(f"sizes/n{n}").offsets)) == [n, n]
    assert sorted(set(np.diff(C.case("sizes/all").offsets))) == sorted(C.SIZES_SMALL)
    m = C.case("mixed/all")
    assert [(int(np.diff(m.offsets)[s]), int(np.diff(m.offsets)[t])) for t, s in m.edges] == list(C.MIXED_PAIRS)
    near = C.case("range/near_r0.6")
    assert np.hypot(near.pts[:, 0], near.pts[:, 1]).max() < 0.1
    assert np.hypot(*C.case("range/far").pts.T).max() > 100.0
    L = C.lattice()
    assert len(L) == 256 and np.all(L * 4 == np.round(L * 4)) and (L == 0).all(1).any()
    S = C.seam_points()
    assert np.signbit(S).any() and (S == 0).all(1).sum() >= 2
    assert [C.case("ratio/r3").max_points(), C.case("ratio/r3").ratio] == [342, 3]
