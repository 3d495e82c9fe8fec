"""ctypes view of the C ABI in include/dpg_slam_c.h and include/dpg_icp_cov.h.

The shared library is dpg-slam_amd/lib/libdpg.so (built by `make -C dpg-slam_amd`, or
`__graft_entry__.build()`).  There is no fallback implementation: if the library is missing,
`lib()` raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DPGSLAM_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libdpg.so")

DPG_OK = 0
DPG_FACTOR_PRIOR = 0
DPG_FACTOR_BETWEEN = 1
DPG_ICP_OK = 0
DPG_ICP_TOO_FEW_CORR = 1
DPG_ICP_LANES = 512


class IcpParams(C.Structure):
    """dpg_icp_params -- PoseGraphParameters ICP fields (parameters.h:105-141)."""

    _fields_ = [
        ("icp_maximum_iterations", C.c_int32),
        ("icp_use_reciprocal_correspondences", C.c_int32),
        ("icp_maximum_transformation_epsilon", C.c_double),
        ("icp_max_correspondence_distance", C.c_double),
        ("ransac_iterations", C.c_int32),
        ("downsample_icp_points_ratio", C.c_int32),
        ("laser_x_variance", C.c_float),
        ("laser_y_variance", C.c_float),
        ("laser_theta_variance", C.c_float),
        ("min_number_correspondences", C.c_int32),
        ("mse_threshold_absolute", C.c_double),
    ]


class IcpResult(C.Structure):
    _fields_ = [
        ("T", C.c_float * 6),
        ("z", C.c_float * 3),
        ("converged", C.c_int32),
        ("iterations", C.c_int32),
        ("n_corr", C.c_int32),
        ("status", C.c_int32),
        ("pad", C.c_int32),
        ("fitness", C.c_double),
    ]


class Factor(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("i", C.c_int32),
        ("j", C.c_int32),
        ("pad", C.c_int32),
        ("z", C.c_double * 3),
        ("info", C.c_double * 3),
    ]


class GnParams(C.Structure):
    _fields_ = [
        ("max_iterations", C.c_int32),
        ("use_error_criteria", C.c_int32),
        ("delta_tol", C.c_double),
        ("relative_error_tol", C.c_double),
        ("absolute_error_tol", C.c_double),
        ("pcg_rel_tol", C.c_double),
        ("pcg_max_iterations", C.c_int32),
        ("pcg_check_every", C.c_int32),
        ("linear_solver", C.c_int32),
        ("reuse_factorization", C.c_int32),
        ("refactor_delta", C.c_double),
    ]


DPG_SOLVER_CHOLESKY = 0
DPG_SOLVER_PCG = 1


class GnStats(C.Structure):
    _fields_ = [
        ("iterations", C.c_int32),
        ("pcg_iterations", C.c_int32),
        ("initial_error", C.c_double),
        ("final_error", C.c_double),
        ("last_delta_inf", C.c_double),
        ("ms_total", C.c_double),
        ("ms_per_iteration", C.c_double),
    ]


class ReoptParams(C.Structure):
    _fields_ = [
        ("max_node_dist_within_pass", C.c_float),
        ("max_node_dist_across_passes", C.c_float),
        ("new_pass_std_dev", C.c_float * 3),
        ("motion_model", C.c_float * 4),
        ("odometry_constraints", C.c_int32),
    ]


class ReoptStats(C.Structure):
    _fields_ = [
        ("n_factors", C.c_int64),
        ("n_icp_edges", C.c_int64),
        ("n_candidates", C.c_int64),
        ("n_loop_closures", C.c_int64),
        ("ms_candidates", C.c_double),
        ("ms_icp", C.c_double),
        ("ms_gn", C.c_double),
        ("gn", GnStats),
    ]


DPG_INC_ISAM2 = 0
DPG_INC_BATCH = 1


class IncParams(C.Structure):
    """dpg_inc_params -- the incremental per-node solve (ISAM2 defaults)."""

    _fields_ = [
        ("mode", C.c_int32),
        ("relinearize_skip", C.c_int32),
        ("relinearize_threshold", C.c_double),
        ("duplicate_factors", C.c_int32),
        ("reorder_every", C.c_int32),
        ("reorder_lead", C.c_int32),
        ("full_refactor", C.c_int32),
        ("gn", GnParams),
    ]


class SolverOptions(C.Structure):
    """dpg_solver_options -- the supernodal Cholesky's options (per context)."""

    _fields_ = [(n, C.c_int32) for n in ("order", "fused", "solve_stage", "solve_maxseg", "solve_dinv",
                                          "merge_single", "max_supernode_cols", "solve_inv_cols")] + [("relax_fraction", C.c_double)]


class IncStats(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_int64),
        ("n_factors", C.c_int64),
        ("nnz_l", C.c_int64),
        ("reordered", C.c_int32),
        ("relinearized", C.c_int32),
        ("gn_iterations", C.c_int32),
        ("fronts_kept", C.c_int32),
        ("error", C.c_double),
        ("last_delta_inf", C.c_double),
        ("ms_total", C.c_double),
        ("ms_symbolic", C.c_double),
        ("ms_numeric", C.c_double),
    ]


class AddNodeStats(C.Structure):
    _fields_ = [
        ("n_icp_edges", C.c_int64),
        ("n_loop_closures", C.c_int64),
        ("ms_icp", C.c_double),
        ("update", IncStats),
    ]


# numpy mirrors of the array-of-struct types (same layout as the C structs)
RESULT_DTYPE = np.dtype(
    [("T", "<f4", (6,)), ("z", "<f4", (3,)), ("converged", "<i4"), ("iterations", "<i4"),
     ("n_corr", "<i4"), ("status", "<i4"), ("pad", "<i4"), ("fitness", "<f8")], align=True)
FACTOR_DTYPE = np.dtype(
    [("kind", "<i4"), ("i", "<i4"), ("j", "<i4"), ("pad", "<i4"), ("z", "<f8", (3,)),
     ("info", "<f8", (3,))], align=True)
assert RESULT_DTYPE.itemsize == C.sizeof(IcpResult) == 64
assert FACTOR_DTYPE.itemsize == C.sizeof(Factor) == 64

P = C.c_void_p
F32P = C.POINTER(C.c_float)
F64P = C.POINTER(C.c_double)
I32P = C.POINTER(C.c_int32)
I64P = C.POINTER(C.c_int64)
U8P = C.POINTER(C.c_uint8)
I8P = C.POINTER(C.c_int8)

# name -> (restype, argtypes); the full exported surface of include/*.h

class ChangeParams(C.Structure):
    """dpg_change_params -- DpgParameters (parameters.h:37-87) + the laser pose (parameters.h:319-339)."""

    _fields_ = [
        ("num_sectors", C.c_int32),
        ("current_pose_chain_len", C.c_int32),
        ("num_bins_for_change_detection", C.c_int32),
        ("pad", C.c_int32),
        ("delta_change_threshold", C.c_double),
        ("current_pose_graph_coverage_threshold", C.c_double),
        ("occ_grid_resolution", C.c_double),
        ("minimum_percent_active_sectors", C.c_float),
        ("distance_threshold_for_local_submap_nodes", C.c_float),
        ("laser", C.c_float * 3),
        ("pad2", C.c_float),
    ]


class ChangeStats(C.Structure):
    """dpg_change_stats -- counters and timings of one dpg_execute_dpg."""

    _fields_ = [(n, C.c_int64) for n in (
        "n_chain", "n_candidates", "n_submap_nodes", "n_chain_cells", "n_uncovered", "n_added", "n_removed",
        "n_committed", "n_sectors_deactivated", "n_nodes_deactivated", "grid_cells", "n_samples")] + [
        ("ms_total", C.c_double), ("ms_kernels", C.c_double)]

    COUNTERS = ("n_chain", "n_candidates", "n_submap_nodes", "n_chain_cells", "n_uncovered", "n_added",
                "n_removed", "n_committed", "n_sectors_deactivated", "n_nodes_deactivated")

    def counters(self) -> dict:
        return {k: int(getattr(self, k)) for k in self.COUNTERS}


class GridParams(C.Structure):
    """dpg_grid_params -- resolution, size bound and margin of dpg_occupancy_grid."""

    _fields_ = [("resolution", C.c_double), ("max_cells", C.c_int64), ("margin_cells", C.c_int32), ("pad", C.c_int32)]


class GridInfo(C.Structure):
    """dpg_grid_info -- the box, counters and timings of one dpg_occupancy_grid."""

    _fields_ = [(n, C.c_int32) for n in ("x0", "y0", "w", "h")] + [("resolution", C.c_double)] + [
        (n, C.c_int64) for n in ("n_nodes_used", "n_beams_used", "n_hits", "n_samples", "n_oob")] + [
        ("ms_total", C.c_double), ("ms_kernels", C.c_double), ("n_direct", C.c_int64), ("n_flushed", C.c_int64)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class CsmParams(C.Structure):
    """dpg_csm_params -- raster, smoothing and search window of the correlative scan matcher."""

    _fields_ = [("resolution", C.c_float), ("sigma", C.c_float), ("kernel_radius", C.c_int32),
                ("half_cells", C.c_int32), ("half_x", C.c_int32), ("half_y", C.c_int32), ("half_a", C.c_int32),
                ("angle_step", C.c_float)]


class CsmResult(C.Structure):
    """dpg_csm_result -- the refined guess of one pair, its score and where in the window it lies."""

    _fields_ = [("guess", C.c_float * 6), ("score", C.c_int32), ("score_at_guess", C.c_int32), ("n_src", C.c_int32),
                ("best_a", C.c_int32), ("best_dx", C.c_int32), ("best_dy", C.c_int32), ("status", C.c_int32),
                ("pad", C.c_int32 * 3)]


CSM_RESULT_DTYPE = np.dtype(
    [("guess", "<f4", (6,)), ("score", "<i4"), ("score_at_guess", "<i4"), ("n_src", "<i4"), ("best_a", "<i4"),
     ("best_dx", "<i4"), ("best_dy", "<i4"), ("status", "<i4"), ("pad", "<i4", (3,))], align=True)
assert CSM_RESULT_DTYPE.itemsize == C.sizeof(CsmResult) == 64 and C.sizeof(CsmParams) == 32
DPG_CSM_OK = 0
DPG_CSM_NO_OVERLAP = 1


class VerifyParams(C.Structure):
    """dpg_verify_params -- raster, occupied radius and sensor position of the loop-closure verification."""

    _fields_ = [("resolution", C.c_float), ("half_cells", C.c_int32), ("occ_radius", C.c_int32),
                ("sensor", C.c_float * 2), ("pad", C.c_int32 * 3)]


class VerifyResult(C.Structure):
    """dpg_verify_result -- per direction the moving cloud's points, those on the table, on occupied and on free cells."""

    _fields_ = [("n_pts", C.c_int32 * 2), ("n_in", C.c_int32 * 2), ("n_support", C.c_int32 * 2),
                ("n_free", C.c_int32 * 2), ("status", C.c_int32), ("pad", C.c_int32 * 7)]


VERIFY_RESULT_DTYPE = np.dtype(
    [("n_pts", "<i4", (2,)), ("n_in", "<i4", (2,)), ("n_support", "<i4", (2,)), ("n_free", "<i4", (2,)),
     ("status", "<i4"), ("pad", "<i4", (7,))], align=True)
assert VERIFY_RESULT_DTYPE.itemsize == C.sizeof(VerifyResult) == 64 and C.sizeof(VerifyParams) == 32
DPG_VERIFY_OK = 0
DPG_VERIFY_NO_OVERLAP = 1


class LocParams(C.Structure):
    """dpg_loc_params -- field, window and pruning of the localisation in the active map."""

    _fields_ = [("resolution", C.c_double), ("max_cells", C.c_int64), ("margin_cells", C.c_int32), ("sigma", C.c_float),
                ("kernel_radius", C.c_int32), ("occupied_min", C.c_int32), ("half_x", C.c_int32), ("half_y", C.c_int32),
                ("half_a", C.c_int32), ("angle_step", C.c_float), ("coarse_shift", C.c_int32),
                ("max_refine_blocks", C.c_int32)]


class LocResult(C.Structure):
    """dpg_loc_result -- the pose of one scan in the active map and how the search found it."""

    _fields_ = [("pose", C.c_float * 3), ("rot", C.c_float * 2), ("score", C.c_int32), ("score_at_guess", C.c_int32),
                ("n_pts", C.c_int32), ("best_a", C.c_int32), ("best_dx", C.c_int32), ("best_dy", C.c_int32),
                ("status", C.c_int32), ("n_seeds", C.c_int32), ("box", C.c_int32 * 4), ("pad", C.c_int32),
                ("n_blocks", C.c_int64), ("n_frontier", C.c_int64), ("n_refined_candidates", C.c_int64),
                ("ms_kernels", C.c_double), ("ms_field", C.c_double), ("ms_bound", C.c_double), ("ms_fine", C.c_double)]


LOC_RESULT_DTYPE = np.dtype(
    [("pose", "<f4", (3,)), ("rot", "<f4", (2,)), ("score", "<i4"), ("score_at_guess", "<i4"), ("n_pts", "<i4"),
     ("best_a", "<i4"), ("best_dx", "<i4"), ("best_dy", "<i4"), ("status", "<i4"), ("n_seeds", "<i4"),
     ("box", "<i4", (4,)), ("pad", "<i4"), ("n_blocks", "<i8"), ("n_frontier", "<i8"), ("n_refined_candidates", "<i8"),
     ("ms_kernels", "<f8"), ("ms_field", "<f8"), ("ms_bound", "<f8"), ("ms_fine", "<f8")], align=True)
assert LOC_RESULT_DTYPE.itemsize == C.sizeof(LocResult) == 128 and C.sizeof(LocParams) == 56
# the fields of a record that two runs of one request share (everything but the timings)
LOC_RESULT_EXACT = tuple(n for n in LOC_RESULT_DTYPE.names if not n.startswith("ms_"))
DPG_LOC_OK = 0
DPG_LOC_NO_OVERLAP = 1
DPG_LOC_UNPROVEN = 2


class FmapInfo(C.Structure):
    """dpg_fmap_info -- what a frozen map holds."""

    _fields_ = [("box", C.c_int32 * 4), ("res", C.c_double), ("sigma", C.c_float), ("kernel_radius", C.c_int32),
                ("occupied_min", C.c_int32), ("pad", C.c_int32), ("n_bytes", C.c_int64)]


class TrackParams(C.Structure):
    """dpg_track_params -- the window of dpg_fmap_track around each scan's guess."""

    _fields_ = [("half_x", C.c_int32), ("half_y", C.c_int32), ("half_a", C.c_int32), ("angle_step", C.c_float)]


class TrackResult(C.Structure):
    """dpg_track_result -- the pose of one scan of a tracked batch."""

    _fields_ = [("pose", C.c_float * 3), ("rot", C.c_float * 2), ("score", C.c_int32), ("score_at_guess", C.c_int32),
                ("n_pts", C.c_int32), ("best_a", C.c_int32), ("best_dx", C.c_int32), ("best_dy", C.c_int32),
                ("status", C.c_int32)]


TRACK_RESULT_DTYPE = np.dtype(
    [("pose", "<f4", (3,)), ("rot", "<f4", (2,)), ("score", "<i4"), ("score_at_guess", "<i4"), ("n_pts", "<i4"),
     ("best_a", "<i4"), ("best_dx", "<i4"), ("best_dy", "<i4"), ("status", "<i4")], align=True)
assert TRACK_RESULT_DTYPE.itemsize == C.sizeof(TrackResult) == 48 and C.sizeof(TrackParams) == 16
assert C.sizeof(FmapInfo) == 48
FMAP_HEADER_SIZE = 64


class RefineParams(C.Structure):
    """dpg_refine_params -- the Gauss-Newton refinement on a frozen map's field (dpg_fmap_refine)."""

    _fields_ = [("max_iters", C.c_int32), ("pad", C.c_int32), ("lambda_", C.c_double), ("max_step_cells", C.c_double),
                ("max_step_angle", C.c_double), ("tol_cells", C.c_double), ("tol_angle", C.c_double)]


class RefineResult(C.Structure):
    """dpg_refine_result -- the refined pose of one scan with its curvature and covariance."""

    _fields_ = [("pose", C.c_float * 3), ("rot", C.c_float * 2), ("status", C.c_int32), ("n_evals", C.c_int32),
                ("best_eval", C.c_int32), ("n_used", C.c_int32), ("pad", C.c_int32), ("tu", C.c_double), ("tv", C.c_double),
                ("c", C.c_double), ("s", C.c_double), ("cost", C.c_double), ("cost_start", C.c_double),
                ("sum_r", C.c_double), ("hess", C.c_double * 6), ("cov", C.c_double * 6), ("cov_ok", C.c_int32),
                ("pad2", C.c_int32)]


REFINE_RESULT_DTYPE = np.dtype(
    [("pose", "<f4", (3,)), ("rot", "<f4", (2,)), ("status", "<i4"), ("n_evals", "<i4"), ("best_eval", "<i4"),
     ("n_used", "<i4"), ("pad", "<i4"), ("tu", "<f8"), ("tv", "<f8"), ("c", "<f8"), ("s", "<f8"), ("cost", "<f8"),
     ("cost_start", "<f8"), ("sum_r", "<f8"), ("hess", "<f8", (6,)), ("cov", "<f8", (6,)), ("cov_ok", "<i4"),
     ("pad2", "<i4")], align=True)
assert REFINE_RESULT_DTYPE.itemsize == C.sizeof(RefineResult) == 200 and C.sizeof(RefineParams) == 48
REFINE_TRACE_COLS = 16
DPG_REFINE_CONVERGED = 0
DPG_REFINE_MAX_ITERS = 1
DPG_REFINE_DEGENERATE = 2
DPG_REFINE_NO_POINTS = 3


ALLREDUCE_F64 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64)
ALLREDUCE_F32 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_int64)
ALLGATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)


class CollOps(C.Structure):
    """dpg_coll_ops -- the caller's blocking host-memory collectives (dpg_ctx_create_rank_ops)."""

    _fields_ = [("user", C.c_void_p), ("allreduce_sum_f64", ALLREDUCE_F64), ("allreduce_sum_f32", ALLREDUCE_F32),
                ("allgather", ALLGATHER)]


SIGNATURES = {
    "dpg_last_error": (C.c_char_p, []),
    "dpg_version": (C.c_char_p, []),
    "dpg_icp_params_default": (None, [C.POINTER(IcpParams)]),
    "dpg_gn_params_default": (None, [C.POINTER(GnParams)]),
    "dpg_ctx_create": (P, [C.c_int]),
    "dpg_ctx_create_multi": (P, [C.c_int32, I32P]),
    "dpg_ctx_num_gpus": (C.c_int32, [P]),
    "dpg_ctx_create_virtual": (P, [C.c_int32, C.c_int32]),
    "dpg_ctx_create_rank": (P, [C.c_int32, P, C.c_int32, C.c_int32]),
    "dpg_ctx_create_rank_ops": (P, [C.c_int32, C.POINTER(CollOps), C.c_int32, C.c_int32]),
    "dpg_shard_plan": (C.c_int, [F32P, C.c_int64, C.c_int32, I32P, I64P, I64P]),
    "dpg_shard_reassemble": (C.c_int, [I32P, C.c_int64, C.c_int32, C.c_int64, C.c_int64, P, P]),
    "dpg_nccl_unique_id": (C.c_int, [P]),
    "dpg_ctx_num_ranks": (C.c_int32, [P]),
    "dpg_ctx_rank": (C.c_int32, [P]),
    "dpg_ctx_set_icp_schedule": (C.c_int, [P, C.c_int32]),
    "dpg_solver_options_default": (None, [C.POINTER(SolverOptions)]),
    "dpg_ctx_set_solver_options": (C.c_int, [P, C.POINTER(SolverOptions)]),
    "dpg_ctx_destroy": (None, [P]),
    "dpg_ctx_set_stream": (C.c_int, [P, P]),
    "dpg_ctx_synchronize": (C.c_int, [P]),
    "dpg_scan_to_cloud": (C.c_int64, [F32P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float,
                                      C.c_float, C.c_float, F32P]),
    "dpg_scans_to_clouds": (C.c_int64, [F32P, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_float,
                                        C.c_float, C.c_float, C.c_float, F32P, I64P]),
    "dpg_downsample_cloud": (C.c_int64, [F32P, C.c_int64, C.c_int32, F32P]),
    "dpg_inverse_transform_point": (None, [F32P, F32P, F32P]),
    "dpg_transform_point": (None, [F32P, F32P, F32P]),
    "dpg_icp_guess": (None, [F32P, F32P, F32P]),
    "dpg_odometry_factors": (C.c_int, [F32P, C.c_int64, I32P, I32P, C.c_int64, C.c_float, C.c_float, C.c_float,
                                      C.c_float, C.c_void_p]),
    "dpg_odometry_factor": (C.c_int, [F32P, F32P, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float,
                                      C.c_float, C.POINTER(Factor)]),
    "dpg_icp_factor": (None, [C.POINTER(IcpResult), C.c_int32, C.c_int32, C.POINTER(IcpParams),
                              C.POINTER(Factor)]),
    "dpg_synth_world": (C.c_int64, [C.c_uint64, C.c_float, F32P, C.c_int64]),
    "dpg_synth_trajectory": (C.c_int, [C.c_uint64, C.c_int64, F32P, C.c_int64, C.c_float, C.c_float, F64P]),
    "dpg_synth_scans": (C.c_int, [F64P, C.c_int64, F32P, C.c_int64, C.c_int32, C.c_float, C.c_float,
                                  C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint64,
                                  C.c_int32, F32P]),
    "dpg_run_icp": (C.c_int, [P, F32P, C.c_int64, F32P, C.c_int64, F32P, F32P, C.POINTER(IcpParams),
                              C.POINTER(IcpResult), F64P, F64P]),
    "dpg_scans_upload": (C.c_int, [P, F32P, I64P, C.c_int64, C.c_int32]),
    "dpg_icp_batch_prepare": (C.c_int, [P, I32P, C.c_int64, F32P, C.POINTER(IcpParams)]),
    "dpg_icp_batch_run": (C.c_int, [P, C.c_int32, C.c_int32]),
    "dpg_icp_batch_fetch": (C.c_int, [P, P, F64P, C.c_int64]),
    "dpg_icp_batch_fetch_trace": (C.c_int, [P, I32P, C.c_int64, I64P]),
    "dpg_icp_batch_size": (C.c_int64, [P]),
    "dpg_icp_batch_kernel_ms": (C.c_float, [P]),
    "dpg_cov_batch_kernel_ms": (C.c_float, [P]),
    "dpg_cov_batch_overlapped": (C.c_int32, [P]),
    "dpg_kdtree_build_ms": (C.c_float, [P]),
    "dpg_ctx_set_icp_variant": (C.c_int, [P, C.c_int32]),
    "dpg_ctx_set_icp_defer_cap": (C.c_int, [P, C.c_int32]),
    "dpg_ctx_set_cov_workgroups": (C.c_int, [P, C.c_int32]),
    "dpg_ctx_set_icp_kernel_variant": (C.c_int, [P, C.c_int32]),
    "dpg_icp_batch_algorithmic_bytes": (C.c_double, [P]),
    "dpg_optimize_graph": (C.c_int, [P, F64P, C.c_int64, P, C.c_int64, C.POINTER(GnParams),
                                     C.POINTER(GnStats)]),
    "dpg_gn_setup": (C.c_int, [P, C.c_int64, P, C.c_int64, C.c_int64, C.c_int64, C.POINTER(GnParams)]),
    "dpg_gn_take_icp_measurements": (C.c_int, [P, C.c_int64, C.c_int64, C.c_int64, C.POINTER(IcpParams)]),
    "dpg_gn_hb_size": (C.c_int64, [P]),
    "dpg_gn_setup_profile": (C.c_int, [P, F64P]),
    "dpg_gn_set_poses": (C.c_int, [P, F64P]),
    "dpg_gn_get_poses": (C.c_int, [P, F64P]),
    "dpg_gn_assemble": (C.c_int, [P, P]),
    "dpg_gn_solve_retract": (C.c_int, [P, P, F64P, F64P, I32P]),
    "dpg_gn_solve_retract_async": (C.c_int, [P, P]),
    "dpg_gn_fetch": (C.c_int, [P, P, F64P]),
    "dpg_gn_factorizations": (C.c_int32, [P]),
    "dpg_gn_run": (C.c_int, [P, F64P, C.POINTER(GnStats)]),
    "dpg_gn_last_assemble_ms": (C.c_float, [P]),
    "dpg_gn_last_solve_ms": (C.c_float, [P]),
    "dpg_gn_marginals": (C.c_int, [P, I32P, C.c_int64, F64P]),
    "dpg_gn_marginal_pairs": (C.c_int, [P, I32P, C.c_int64, F64P]),
    "dpg_gn_cross_covariances": (C.c_int, [P, I32P, C.c_int64, F64P]),
    "dpg_gn_joint_marginal": (C.c_int, [P, I32P, C.c_int64, F64P]),
    "dpg_gn_relative_covariances": (C.c_int, [P, I32P, C.c_int64, F64P]),
    "dpg_gn_joint_profile": (C.c_int, [P, I32P, C.c_int64, F64P, C.c_int64]),
    "dpg_marginal_covariances": (C.c_int, [P, F64P, C.c_int64, P, C.c_int64, I32P, C.c_int64, F64P]),
    "dpg_gn_marginals_profile": (C.c_int64, [P, F64P, C.c_int64]),
    "icp_cov_calculate": (C.c_int, [P, F32P, C.c_int64, F32P, C.c_int64, F32P, C.c_float, C.c_float,
                                    C.c_float, F64P, F64P]),
    "icp_cov_sandwich": (C.c_int, [P, F32P, C.c_int64, F32P, C.c_int64, F32P, F64P, F64P]),
    "dpg_reopt_params_default": (None, [C.POINTER(ReoptParams)]),
    "dpg_get_map": (C.c_int64, [P, F32P, C.c_int32, F32P, C.c_int64]),
    "dpg_get_map_kernel_ms": (C.c_float, [P]),
    "dpg_loop_closure_candidates": (C.c_int64, [P, C.c_int64, I32P, F32P, C.c_float, C.c_float, I32P, C.c_int64]),
    "dpg_change_params_default": (None, [C.POINTER(ChangeParams)]),
    "dpg_dpg_create": (P, [P, C.c_int64, I64P, F32P, F32P, C.POINTER(ChangeParams)]),
    "dpg_dpg_destroy": (None, [P]),
    "dpg_dpg_append": (C.c_int, [P, C.c_int64, I64P, F32P, F32P]),
    "dpg_execute_dpg": (C.c_int, [P, C.c_int64, C.c_int64, F32P, C.POINTER(ChangeStats)]),
    "dpg_execute_dpg_chain": (C.c_int, [P, C.c_int64, C.c_int64, F32P, F32P, C.POINTER(ChangeStats)]),
    "dpg_dpg_fetch": (C.c_int, [P, U8P, U8P, U8P]),
    "dpg_dpg_load": (C.c_int, [P, U8P, U8P, U8P]),
    "dpg_active_dynamic_points": (C.c_int64, [P, C.c_int64, F32P, F32P, C.c_int64, I64P]),
    "dpg_grid_params_default": (None, [C.POINTER(GridParams)]),
    "dpg_occupancy_grid": (C.c_int, [P, C.c_int64, F32P, C.POINTER(GridParams), I32P, I32P, I8P, C.c_int64,
                                     C.POINTER(GridInfo)]),
    "dpg_dpg_beam_geometry": (C.c_int, [P, C.c_int64, F32P, F32P, F32P, C.c_int64]),
    "dpg_occupancy_from_counts": (None, [I32P, I32P, C.c_int64, I8P]),
    "dpg_grid_box": (C.c_int, [F32P, F32P, U8P, C.c_int64, C.c_double, C.c_int32, I32P]),
    "dpg_csm_params_default": (None, [C.POINTER(CsmParams)]),
    "dpg_csm_lds_bytes": (C.c_int64, [C.POINTER(CsmParams)]),
    "dpg_csm_lut": (C.c_int, [C.POINTER(CsmParams), U8P]),
    "dpg_csm_rotations": (C.c_int, [F32P, C.POINTER(CsmParams), F32P]),
    "dpg_csm_batch": (C.c_int, [P, I32P, C.c_int64, F32P, F32P, C.POINTER(CsmParams), P, C.c_int64]),
    "dpg_csm_table": (C.c_int, [P, C.c_int32, C.POINTER(CsmParams), U8P, C.c_int64]),
    "dpg_csm_scores": (C.c_int, [P, C.c_int32, C.c_int32, F32P, C.POINTER(CsmParams), I32P, C.c_int64]),
    "dpg_csm_kernel_ms": (C.c_float, [P]),
    "dpg_icp_batch_prepare_guess": (C.c_int, [P, I32P, C.c_int64, F32P, C.POINTER(IcpParams)]),
    "dpg_verify_params_default": (None, [C.POINTER(VerifyParams)]),
    "dpg_verify_params_check": (C.c_int, [C.POINTER(VerifyParams)]),
    "dpg_verify_lds_bytes": (C.c_int64, [C.POINTER(VerifyParams)]),
    "dpg_verify_sensor_key": (C.c_int, [C.POINTER(VerifyParams), I32P]),
    "dpg_verify_batch": (C.c_int, [P, I32P, C.c_int64, F32P, C.POINTER(VerifyParams), P, C.c_int64]),
    "dpg_verify_table": (C.c_int, [P, C.c_int32, C.POINTER(VerifyParams), U8P, C.c_int64]),
    "dpg_verify_kernel_ms": (C.c_float, [P]),
    "dpg_loc_params_default": (None, [C.POINTER(LocParams)]),
    "dpg_loc_params_check": (C.c_int, [C.POINTER(LocParams)]),
    "dpg_loc_rotations": (C.c_int, [C.c_float, C.POINTER(LocParams), F32P]),
    "dpg_map_localize": (C.c_int, [P, C.c_int64, F32P, F32P, C.c_int64, F32P, C.POINTER(LocParams),
                                   C.POINTER(LocResult)]),
    "dpg_map_field": (C.c_int, [P, C.c_int64, F32P, C.POINTER(LocParams), C.c_int32, U8P, C.c_int64, I32P]),
    "dpg_map_localize_bounds": (C.c_int, [P, C.c_int64, F32P, F32P, C.c_int64, F32P, C.POINTER(LocParams), I32P,
                                          C.c_int64]),
    "dpg_map_localize_scores": (C.c_int, [P, C.c_int64, F32P, F32P, C.c_int64, F32P, C.POINTER(LocParams), I32P,
                                          C.c_int64]),
    "dpg_fmap_create": (P, [P, C.c_int64, F32P, C.POINTER(LocParams)]),
    "dpg_fmap_from_field": (P, [P, U8P, I32P, C.c_double, C.c_float, C.c_int32, C.c_int32]),
    "dpg_fmap_info_get": (C.c_int, [P, C.POINTER(FmapInfo)]),
    "dpg_fmap_fetch": (C.c_int, [P, U8P, C.c_int64]),
    "dpg_fmap_destroy": (None, [P]),
    "dpg_fmap_save": (C.c_int, [P, C.c_char_p]),
    "dpg_fmap_load": (P, [P, C.c_char_p]),
    "dpg_fmap_header_check": (C.c_int, [C.c_void_p, C.c_int64]),
    "dpg_fmap_localize": (C.c_int, [P, F32P, C.c_int64, F32P, C.POINTER(LocParams), C.POINTER(LocResult)]),
    "dpg_track_params_default": (None, [C.POINTER(TrackParams)]),
    "dpg_track_params_check": (C.c_int, [C.POINTER(TrackParams)]),
    "dpg_fmap_track": (C.c_int, [P, F32P, I64P, C.c_int64, F32P, C.POINTER(TrackParams), P]),
    "dpg_fmap_track_kernel_ms": (C.c_float, [P]),
    "dpg_refine_params_default": (None, [C.POINTER(RefineParams)]),
    "dpg_refine_params_check": (C.c_int, [C.POINTER(RefineParams)]),
    "dpg_refine_start": (C.c_int, [F32P, F32P]),
    "dpg_refine_angle": (C.c_float, [C.c_double, C.c_double]),
    "dpg_fmap_refine": (C.c_int, [P, F32P, I64P, C.c_int64, F32P, C.POINTER(RefineParams), P]),
    "dpg_fmap_refine_trace": (C.c_int, [P, F32P, I64P, C.c_int64, F32P, C.POINTER(RefineParams), P, F64P, C.c_int64]),
    "dpg_fmap_track_refine": (C.c_int, [P, F32P, I64P, C.c_int64, F32P, C.POINTER(TrackParams), C.POINTER(RefineParams),
                                        P, P]),
    "dpg_fmap_refine_kernel_ms": (C.c_float, [P]),
    "dpg_reoptimize": (C.c_int, [P, C.c_int64, I32P, F32P, F32P, C.POINTER(IcpParams), C.POINTER(GnParams),
                                 C.POINTER(ReoptParams), F64P, C.POINTER(ReoptStats)]),
    "dpg_reoptimize_inc": (C.c_int, [P, C.c_int64, I32P, F32P, F32P, C.POINTER(IcpParams), C.POINTER(ReoptParams),
                                     F64P, C.POINTER(ReoptStats)]),
    "dpg_inc_params_default": (None, [C.POINTER(IncParams)]),
    "dpg_inc_create": (P, [P, C.POINTER(IncParams)]),
    "dpg_inc_destroy": (None, [P]),
    "dpg_inc_reset": (C.c_int, [P]),
    "dpg_inc_update": (C.c_int, [P, C.c_int64, F64P, P, C.c_int64, C.POINTER(IncStats)]),
    "dpg_inc_num_nodes": (C.c_int64, [P]),
    "dpg_inc_get_poses": (C.c_int, [P, F64P, C.c_int64]),
    "dpg_inc_marginals": (C.c_int, [P, I32P, C.c_int64, F64P]),
    "dpg_inc_cross_covariances": (C.c_int, [P, I32P, C.c_int64, F64P]),
    "dpg_inc_joint_marginal": (C.c_int, [P, I32P, C.c_int64, F64P]),
    "dpg_inc_relative_covariances": (C.c_int, [P, I32P, C.c_int64, F64P]),
    "dpg_inc_save": (C.c_int, [P, C.c_char_p]),
    "dpg_inc_load": (P, [P, C.c_char_p]),
    "dpg_inc_export": (C.c_int64, [P, I64P, P, I32P, C.c_int64, F64P, F64P, F64P]),
    "dpg_scans_append": (C.c_int, [P, F32P, I64P, C.c_int64, C.c_int32]),
    "dpg_add_node": (C.c_int, [P, F32P, C.c_int64, I32P, F32P, P, C.c_int64, C.POINTER(IcpParams),
                               C.POINTER(ReoptParams), C.c_int32, C.POINTER(AddNodeStats)]),
    "dpg_add_node_pairs": (C.c_int, [P, F32P, C.c_int64, F32P, P, C.c_int64, I32P, C.c_int64, C.c_int32,
                                     C.POINTER(IcpParams), C.POINTER(AddNodeStats)]),
}


def default_inc_params() -> IncParams:
    p = IncParams()
    lib().dpg_inc_params_default(C.byref(p))
    return p


def default_solver_options() -> SolverOptions:
    o = SolverOptions()
    lib().dpg_solver_options_default(C.byref(o))
    return o


def default_reopt_params() -> ReoptParams:
    p = ReoptParams()
    lib().dpg_reopt_params_default(C.byref(p))
    return p

_LIB = None


def lib() -> C.CDLL:
    """Load libdpg.so (raises OSError/RuntimeError when it is not built -- no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is not built; run `make -C dpg-slam_amd` or __graft_entry__.build()")
        # One HIP runtime per process: PyTorch ships its own libamdhip64 (same soname), so load it
        # first and libdpg binds to it; loaded the other way round torch would bring a second
        # runtime that finds no GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def ptr(a: np.ndarray, ctype):
    """Pointer to a contiguous numpy array (None for None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
    return a.ctypes.data_as(C.POINTER(ctype))


def vptr(a: np.ndarray):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return C.c_void_p(a.ctypes.data)


class DpgError(RuntimeError):
    pass


def check(rc: int, what: str = "dpg call"):
    if rc != DPG_OK:
        msg = lib().dpg_last_error()
        raise DpgError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def default_icp_params() -> IcpParams:
    p = IcpParams()
    lib().dpg_icp_params_default(C.byref(p))
    return p


def default_change_params() -> ChangeParams:
    p = ChangeParams()
    lib().dpg_change_params_default(C.byref(p))
    return p


default_change_params_host = default_change_params


def default_grid_params() -> GridParams:
    p = GridParams()
    lib().dpg_grid_params_default(C.byref(p))
    return p


def default_csm_params() -> CsmParams:
    p = CsmParams()
    lib().dpg_csm_params_default(C.byref(p))
    return p


def default_verify_params() -> VerifyParams:
    p = VerifyParams()
    lib().dpg_verify_params_default(C.byref(p))
    return p


def default_loc_params() -> LocParams:
    p = LocParams()
    lib().dpg_loc_params_default(C.byref(p))
    return p


def default_track_params() -> TrackParams:
    p = TrackParams()
    lib().dpg_track_params_default(C.byref(p))
    return p


def default_refine_params() -> RefineParams:
    p = RefineParams()
    lib().dpg_refine_params_default(C.byref(p))
    return p


def default_gn_params() -> GnParams:
    p = GnParams()
    lib().dpg_gn_params_default(C.byref(p))
    return p
