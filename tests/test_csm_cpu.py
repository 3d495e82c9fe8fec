"""Correlative scan matching, host side (no GPU): the numpy reference (tests/csm_ref.py) pinned by
hand, the host functions of dpg_host.c (smoothing bytes, rotations, parameter and LDS checks), the
ABI structs against the header compiled as C, DpgSLAM's backend protocol, and the reference alone
recovering a known offset on the room the GPU end-to-end test reuses."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import csm_ref as R
from dpgslam import _abi, api
from dpgslam._abi import lib, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
ERR_ARG = -1   # DPG_ERR_ARG
DEFAULT_LUT = [255, 155, 94, 57, 35, 21, 13, 8, 5, 3]


def _params(**kw):
    p = _abi.default_csm_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_reference_one_target_point_is_the_stencil():
    """One target point at key (2, -1): the table is lut[d2] around it, 0 beyond R."""
    p = _params(half_cells=6)
    T = R.table(np.array([[0.2, -0.1]], np.float32), p, np.array(DEFAULT_LUT, np.uint8))
    assert T.shape == (13, 13)
    for v in range(-6, 7):
        for u in range(-6, 7):
            d2 = (u - 2) ** 2 + (v + 1) ** 2
            assert T[v + 6, u + 6] == (DEFAULT_LUT[d2] if d2 <= 9 else 0), (u, v)
    # a point outside the table still spreads into it; duplicates change nothing; non-finite and huge points count for nothing
    T2 = R.table(np.array([[0.8, 0.0], [0.8, 0.0], [np.nan, 0.0], [0.0, np.inf], [6e7, 0.0]], np.float32), p,
                 np.array(DEFAULT_LUT, np.uint8))
    assert T2[6, 12] == DEFAULT_LUT[4] and T2[6, 11] == DEFAULT_LUT[9] and T2[6, 10] == 0 and T2.sum() == T2[:, 11:].sum()
    # halves round away from zero, both signs
    assert R.c_round([0.5, 1.5, 2.5, -0.5, -1.5, 0.49999999999999994, -2.5]).tolist() == [1, 2, 3, -1, -2, 0, -3]
    kx, ky, ok = R.keys(np.array([[0.25, -0.25], [0.75, -0.75]], np.float32), 0.5)
    assert kx.tolist() == [1, 2] and ky.tolist() == [-1, -2] and ok.all()


def test_reference_one_source_point_is_the_shifted_table():
    """One source point at key (1, 2) under the identity guess: score(a = centre, dx, dy) = T[1 + dx, 2 + dy],
    0 where the shifted cell leaves the table."""
    p = _params(half_cells=4, half_x=3, half_y=5, half_a=0)
    rng = np.random.default_rng(3)
    T = rng.integers(0, 256, (9, 9)).astype(np.uint8)
    vol = R.scores(T, np.array([[0.1, 0.2]], np.float32), R.guess_of(0, 0, 0), p, np.array([[1.0, 0.0]], np.float32))
    assert vol.shape == (1, 11, 7)
    for dy in range(-5, 6):
        for dx in range(-3, 4):
            u, v = 1 + dx, 2 + dy
            want = int(T[v + 4, u + 4]) if abs(u) <= 4 and abs(v) <= 4 else 0
            assert vol[0, dy + 5, dx + 3] == want, (dx, dy)


def test_reference_tie_order_on_a_plateau():
    p = _params(half_x=2, half_y=2, half_a=2)
    vol = np.zeros((5, 5, 5), np.int32)
    assert R.winner(vol, p) == (2, 0, 0)                     # all equal: the guess itself
    vol[:] = 0
    vol[0, 2, 2] = vol[4, 2, 2] = 7                          # |a - ha| equal, d2 equal: the smaller a
    assert R.winner(vol, p) == (0, 0, 0)
    vol[1, 0, 0] = 7                                         # a smaller |a - ha| beats a smaller d2
    assert R.winner(vol, p) == (1, -2, -2)
    vol[:] = 0
    vol[2, 2, 3] = vol[2, 3, 2] = vol[2, 1, 2] = vol[2, 2, 1] = 5   # d2 = 1 four times: smaller dy, then smaller dx
    assert R.winner(vol, p) == (2, 0, -1)
    vol[2, 1, 2] = 0
    assert R.winner(vol, p) == (2, -1, 0)                    # dy = 0 twice: the smaller dx
    vol[3, 4, 4] = 6                                         # the score comes first
    assert R.winner(vol, p) == (3, 2, 2)


def test_lut_defaults_and_radius_zero():
    assert api.csm_lut().tolist() == DEFAULT_LUT
    assert api.csm_lut(_params(kernel_radius=0)).tolist() == [255]
    lut = api.csm_lut(_params(kernel_radius=7, sigma=0.25))
    assert len(lut) == 50 and lut[0] == 255 and (np.diff(lut.astype(int)) <= 0).all()
    # the formula in double with the floats widened
    res, sig = float(np.float32(0.1)), float(np.float32(0.25))
    assert lut.tolist() == [int(math.floor(255.0 * math.exp(-d2 * res * res / (2.0 * sig * sig)) + 0.5)) for d2 in range(50)]


def test_rotations():
    g = R.guess_of(0.3, -0.2, 0.7)
    r0 = api.csm_rotations(g, _params(half_a=0))
    th = math.atan2(float(g[3]), float(g[0]))
    assert r0.shape == (1, 2) and r0[0].tolist() == [np.float32(math.cos(th)), np.float32(math.sin(th))]
    p = _params(half_a=3)
    r = api.csm_rotations(g, p)
    assert r.shape == (7, 2) and r[3].tolist() == r0[0].tolist()
    want = [[np.float32(math.cos(th + (a - 3) * float(p.angle_step))), np.float32(math.sin(th + (a - 3) * float(p.angle_step)))]
            for a in range(7)]
    assert np.abs(r - np.array(want, np.float32)).max() <= 1.2e-7   # libm's cos / sin: within one float ulp


def test_defaults_and_struct_layouts_match_the_header(tmp_path):
    p = _abi.default_csm_params()
    assert (p.resolution, p.sigma) == (np.float32(0.1), np.float32(0.1))
    assert (p.kernel_radius, p.half_cells, p.half_x, p.half_y, p.half_a) == (3, 160, 15, 15, 20)
    assert p.angle_step == np.float32(0.5 * math.pi / 180.0)
    txt = open(os.path.join(INC, "dpg_slam_c.h")).read()
    sizes = {k: int(v) for k, v in re.findall(r"#define (DPG_CSM_\w+) (\d+)", txt)}
    assert len(re.findall(r"_Static_assert\(sizeof\(dpg_csm_params\) == DPG_CSM_PARAMS_SIZE && "
                          r"sizeof\(dpg_csm_result\) == DPG_CSM_RESULT_SIZE", txt)) == 1
    assert C.sizeof(_abi.CsmParams) == sizes["DPG_CSM_PARAMS_SIZE"] == 32
    assert C.sizeof(_abi.CsmResult) == sizes["DPG_CSM_RESULT_SIZE"] == 64 == _abi.CSM_RESULT_DTYPE.itemsize
    for struct, cls in (("dpg_csm_params", _abi.CsmParams), ("dpg_csm_result", _abi.CsmResult)):
        names = [f[0] for f in cls._fields_]
        body = "".join(f'printf(" %zu", offsetof({struct}, {f}));' for f in names)
        src = tmp_path / f"{struct}.c"
        src.write_text(f'#include <stddef.h>\n#include <stdio.h>\n#include "dpg_slam_c.h"\n'
                       f'int main(void) {{ printf("%zu", sizeof({struct})); {body} return 0; }}\n')
        exe = str(tmp_path / struct)
        subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", INC, "-o", exe, str(src)], check=True)
        lay = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
        assert lay[0] == C.sizeof(cls)
        assert lay[1:] == [getattr(cls, n).offset for n in names]
        if struct == "dpg_csm_result":   # the numpy mirror too
            assert lay[1:] == [_abi.CSM_RESULT_DTYPE.fields[n][1] for n in names]
    # the LDS formula of the header comment
    fixed, budget = sizes["DPG_CSM_LDS_FIXED"], sizes["DPG_CSM_LDS_BUDGET"]
    assert budget == 160 * 1024
    assert api.csm_lds_bytes(p) == (381 * 381 + 15) // 16 * 16 + fixed
    assert api.csm_lds_bytes(_params(half_cells=8, half_x=1, half_y=2)) == (21 * 25 + 15) // 16 * 16 + fixed


def test_parameter_errors():
    bad = [dict(resolution=0.0), dict(resolution=-0.1), dict(resolution=float("nan")), dict(resolution=float("inf")),
           dict(sigma=0.0), dict(sigma=float("nan")), dict(kernel_radius=-1), dict(kernel_radius=8), dict(half_cells=-1),
           dict(half_x=-1), dict(half_x=65), dict(half_y=-1), dict(half_y=65), dict(half_a=-1), dict(half_a=65),
           dict(angle_step=0.0), dict(angle_step=float("nan")),
           dict(half_cells=166), dict(half_cells=2 ** 30), dict(half_cells=100, half_x=64, half_y=64)]   # the LDS budget
    lut = np.zeros(64, np.uint8)
    rot = np.zeros((129, 2), np.float32)
    g = R.guess_of(0, 0, 0)
    for kw in bad:
        p = _params(**kw)
        assert lib().dpg_csm_lds_bytes(C.byref(p)) == ERR_ARG, kw
        assert lib().dpg_csm_lut(C.byref(p), ptr(lut, C.c_uint8)) == ERR_ARG, kw
        assert lib().dpg_csm_rotations(ptr(g, C.c_float), C.byref(p), ptr(rot, C.c_float)) == ERR_ARG, kw
        with pytest.raises(_abi.DpgError):
            api.csm_lds_bytes(p)
    assert lib().dpg_csm_lds_bytes(None) == ERR_ARG
    assert lib().dpg_csm_lut(C.byref(_params()), None) == ERR_ARG
    assert lib().dpg_csm_rotations(None, C.byref(_params()), ptr(rot, C.c_float)) == ERR_ARG
    # the largest table that fits beside the default window, and every limit itself
    assert api.csm_lds_bytes(_params(half_cells=165)) <= 160 * 1024
    assert api.csm_lds_bytes(_params(kernel_radius=7, half_cells=0, half_x=64, half_y=64, half_a=64)) > 0


class _Backend:
    """Aligns from poses only: no prematch, no icp_batch_guess."""

    def candidates(self, est, passes, within, across):
        return np.array([[0, 2]], np.int32)

    def icp_batch(self, clouds, edges, est, p):
        raise AssertionError("the pre-matched sweep must not take the plain path")


def test_slam_prematch_needs_the_backend_methods():
    from dpgslam.slam import DpgSLAM
    s = DpgSLAM(backend=_Backend(), loop_closure_prematch=_abi.default_csm_params())
    s.poses = np.zeros((3, 3), np.float32)
    s.node_pass = np.zeros(3, np.int32)
    with pytest.raises(NotImplementedError, match="prematch"):
        s.reoptimize()
    _Backend.prematch = lambda self, *a: None
    try:
        with pytest.raises(NotImplementedError, match="icp_batch_guess"):
            s.reoptimize()
    finally:
        del _Backend.prematch


def test_reference_recovers_a_known_offset_on_the_room():
    """The room of the GPU end-to-end test: the guess is off by Room.OFFSET (1.77 m, 9.2 degrees), and
    the reference alone puts it back within one cell and one angle step, with a unique winner."""
    rm = R.room()
    p = _abi.default_csm_params()
    assert abs(rm.OFFSET[0]) <= p.half_x * p.resolution and abs(rm.OFFSET[1]) <= p.half_y * p.resolution
    assert abs(rm.OFFSET[2]) <= p.half_a * p.angle_step
    g = api.icp_guess(rm.est[1], rm.est[0])
    e0 = rm.error(R.guess_pose(g))
    assert e0[0] > 1.5 and e0[1] > 0.15
    r, vol = R.result(rm.clouds[0], rm.clouds[1], g, p)
    top = np.sort(vol.ravel())[::-1]
    print(f"winner {int(r['score'])} of {255 * int(r['n_src'])}, runner-up {int(top[1])}, at the guess {int(r['score_at_guess'])}")
    assert top[0] == r["score"] and top[0] > top[1]                  # unique
    assert r["score"] > 5 * r["score_at_guess"] and r["status"] == _abi.DPG_CSM_OK
    e1 = rm.error(R.guess_pose(r["guess"]))
    print(f"error at the guess {e0[0]:.3f} m {math.degrees(e0[1]):.2f} deg, refined {e1[0]:.4f} m {math.degrees(e1[1]):.3f} deg")
    assert e1[0] <= float(p.resolution) * math.sqrt(2.0) and e1[1] <= float(p.angle_step)
