"""DpgSLAM -- the public API of dpg_slam::DpgSLAM (src/dpg_slam/dpg_slam.h:283-335) as a host-side
driver over the MI355X C ABI: the per-node pipeline the ROS glue runs (ObserveOdometry,
ObserveLaser -> updatePoseGraph -> runIcp / optimizeGraph -> executeDPG, incrementPassNumber ->
reoptimize, GetPose, GetMap, getActiveAndDynamicMapPoints).

The bookkeeping (odometry thresholds, node creation, which scans are aligned, which factors are
added) follows dpg_slam.cc line by line in float32 where the reference is float; every numeric
step runs through a backend: GpuBackend (the HIP kernels, dpgslam.api) by default, or any object
with the same methods (tests/slam_oracle.py holds the CPU restatement the tests compare against).
optimizeGraph is the incremental graph (dpg_inc): one ISAM2-semantics update per node by default
(inc_mode="isam2"), or Gauss-Newton to convergence per node (inc_mode="batch"); SURVEY Q1/Q6.
"""
from __future__ import annotations

import ctypes as C
import math

import time

import numpy as np

from . import _abi, api
from ._abi import FACTOR_DTYPE, lib

f32 = np.float32


def _angle_mod(a) -> np.float32:
    """math_utils::AngleMod<float> (math_utils.h:13-16): the subtraction in double."""
    ad = float(f32(a))
    ad -= (math.pi * 2.0) * float(np.rint(ad / (math.pi * 2.0)))
    return f32(ad)


def _icp_factor(res, i, j, p) -> np.ndarray:
    """addObservationConstraint (dpg_slam.cc:331-338) over the ICP result (dpg_icp_factor)."""
    f = _abi.Factor()
    r = _abi.IcpResult.from_buffer_copy(np.ascontiguousarray(res).tobytes()) if isinstance(res, np.ndarray) else res
    lib().dpg_icp_factor(C.byref(r), i, j, C.byref(p), C.byref(f))
    return np.frombuffer(bytes(f), FACTOR_DTYPE).copy()


class GpuBackend:
    """The numeric steps of DpgSLAM on the MI355X (dpgslam.api over the C ABI).  Per node ONE call,
    dpg_add_node: the node's cloud joins the device scan store, its successive and loop-closure
    alignments run as one batched ICP, and the factors go into the incremental graph (dpg_inc)."""

    def __init__(self, ctx: api.Context, inc_mode: str = "isam2"):
        self.ctx = ctx
        self.inc = api.IncGraph(ctx, mode=inc_mode)
        self.stored = 0        # nodes in the context's scan store (dpg_add_node appends each node's cloud)
        self.last_add = None   # AddNodeStats of the last node

    def add_node(self, cloud, passes, init_pose, extra, icp_params, reopt_params, non_successive):
        st = self.inc.add_node(cloud, passes, init_pose, extra, icp_params, reopt_params, non_successive)
        self.stored += 1
        self.last_add = st
        n_icp = (1 if len(passes) > 1 else 0) + int(st.n_loop_closures)
        return n_icp, self.inc.poses()

    def icp_batch(self, clouds, edges, est, p):
        """clouds() -> (pts, offsets) of every node; the store already holds them when every node
        came through add_node."""
        self._ensure_scans(clouds, len(est), p.downsample_icp_points_ratio)
        res, _ = self.ctx.icp_batch(edges, est, p, compute_cov=False)
        return res

    def _ensure_scans(self, clouds, n_nodes, ratio):
        if self.stored != n_nodes:
            pts, offsets = clouds()
            self.ctx.upload_scans(pts, offsets, ratio)
            self.stored = n_nodes

    def prematch(self, clouds, edges, est, csm_params, ratio):
        """The correlative scan match of `edges` from the estimates (dpg_csm_batch)."""
        self._ensure_scans(clouds, len(est), ratio)
        return self.ctx.csm_batch(edges, poses=est, params=csm_params)

    def verify(self, clouds, edges, transforms, params, ratio):
        """The free-space consistency counts of `edges` under their alignments (dpg_verify_batch).  The
        store holds the clouds already when the alignments came from icp_batch / icp_batch_guess."""
        if not self.stored:
            pts, offsets = clouds()
            self._ensure_scans(lambda: (pts, offsets), len(offsets) - 1, ratio)
        return self.ctx.verify_batch(edges, transforms, params)

    def icp_batch_guess(self, clouds, edges, guesses, n_nodes, p):
        """icp_batch with every edge's guess given."""
        self._ensure_scans(clouds, n_nodes, p.downsample_icp_points_ratio)
        res, _ = self.ctx.icp_batch_guess(edges, guesses, p, compute_cov=False)
        return res

    def candidates(self, est, passes, within, across):
        return self.ctx.loop_closure_candidates(est, passes, within, across)

    def rebuild_graph(self, est, F):
        """reoptimize's new ISAM2 + new graph and its one update (dpg_slam.cc:36-39,111-119); the
        scan store holds every node's cloud (icp_batch uploaded them)."""
        self.inc.reset()
        self.last_rebuild = self.inc.update(np.asarray(est, np.float64), F)
        return self.inc.poses()

    def marginals(self, nodes=None):
        """ISAM2::marginalCovariance of the graph as it stands (dpg_inc_marginals): [n, 3, 3]."""
        return self.inc.marginals(nodes)

    def relative_covariances(self, pairs):
        """The covariance of X_i^-1 X_j per node pair (dpg_inc_relative_covariances): [n, 3, 3]."""
        return self.inc.relative_covariances(pairs)

    def store(self, ranges, geom, offsets, params):
        return api.DpgStore(self.ctx, ranges, geom, offsets=offsets, params=params)

    def get_map(self, clouds, est, fraction, ratio):
        self._ensure_scans(clouds, len(est), ratio)
        return self.ctx.get_map(est, fraction)


class DpgSLAM:
    """dpg_slam::DpgSLAM.  Parameters default to parameters.h (PoseGraphParameters, DpgParameters,
    VisualizationParams.display_points_fraction_)."""

    def __init__(self, backend="gpu", ctx: api.Context | None = None, icp_params=None, gn_params=None,
                 change_params=None, min_dist_between_nodes=1.0, min_angle_between_nodes=math.pi / 6.0,
                 non_successive_scan_constraints=True, odometry_constraints=True,
                 max_dist_within_pass=5.0, max_dist_across_passes=2.0, new_pass_std_dev=(0.2, 0.2, 0.15),
                 motion_model=(0.4, 0.4, 0.4, 0.4), display_points_fraction=10, inc_mode="isam2",
                 loop_closure_prematch=None, prematch_min_response=0.0, new_pass_start=None,
                 localize_min_response=0.0, loop_closure_verify=None, verify_max_free_fraction=0.15,
                 verify_min_support_fraction=0.25):
        """loop_closure_prematch: None (the reference's behaviour), or a _abi.CsmParams: reoptimize()
        then runs the correlative scan matcher (dpg_csm_batch) on its loop-closure candidates -- not
        on the successive pairs -- and starts the ICP of a candidate from the matcher's pose where
        score / (255 n_src) >= prematch_min_response, so that a candidate whose estimates drifted
        beyond ICP's correspondence distance can still close.  The per-node path (dpg_add_node, one C
        call per node) is out of scope: it aligns from the estimates as before.

        new_pass_start: None (the reference's behaviour: every pass starts at (0, 0, 0)), or a
        _abi.LocParams: the first scan of every pass >= 1 is localised in the active map before its
        node is created (dpg_map_localize over the whole map; the full circle unless the params narrow
        it).  With status DPG_LOC_OK or DPG_LOC_UNPROVEN and score / (255 n_pts) >=
        localize_min_response the node is created at that pose and the pass's prior carries it as its
        mean, in reoptimize() too; otherwise the node starts at (0, 0, 0) as before.  Every attempt's
        record is kept in last_localization.

        loop_closure_verify: None (the reference's behaviour: every converged loop closure becomes a
        factor), or a _abi.VerifyParams: reoptimize() then checks every loop-closure candidate whose ICP
        converged -- never the successive pairs -- by free-space consistency under that ICP's transform
        (dpg_verify_batch) and keeps it only where api.verify_accept(records, verify_max_free_fraction,
        verify_min_support_fraction) says so; the records and the edges they belong to are kept in
        last_verify.  It works with and without loop_closure_prematch.  The defaults 0.15 / 0.25 come
        from a CPU prototype: true closures of sparse 60-point clouds showed free fractions up to 0.086
        and support from 0.43, a converged alignment 1.4 m off free fractions of 0.23 / 0.27.  They are
        the user's to tune: across passes of a changing environment a true closure legitimately shows
        some free-space hits (a box that moved).  The per-node path (dpg_add_node) is out of scope, as
        it is for the prematch."""
        self.verify_params = loop_closure_verify
        self.verify_max_free = float(verify_max_free_fraction)
        self.verify_min_support = float(verify_min_support_fraction)
        self.last_verify = None                         # (records, edges) of the last sweep's verification
        self.new_pass_start = new_pass_start
        self.localize_min_response = float(localize_min_response)
        self.last_localization = None                   # the record of the last new-pass localisation
        self.pass_start_pose = {}                       # first node of a localised pass -> its prior's mean
        self.prematch_params = loop_closure_prematch
        self.prematch_min_response = float(prematch_min_response)
        self.last_prematch = None                       # the matcher's records of the last sweep
        if backend == "gpu":
            self.ctx = ctx or api.Context(0)
            self.be = GpuBackend(self.ctx, inc_mode)
        elif isinstance(backend, str):
            raise ValueError(f"unknown backend {backend!r} (pass a backend object for anything but 'gpu')")
        else:
            self.be = backend
        self.icp_params = icp_params or _abi.default_icp_params()
        self.gn_params = gn_params or _abi.default_gn_params()
        self.change_params = change_params or _abi.default_change_params()
        self.laser = tuple(float(x) for x in self.change_params.laser)
        self.min_dist = f32(min_dist_between_nodes)
        self.min_angle = f32(min_angle_between_nodes)
        self.non_successive = bool(non_successive_scan_constraints)
        self.odometry_constraints = bool(odometry_constraints)
        self.within, self.across = f32(max_dist_within_pass), f32(max_dist_across_passes)
        self.prior_sigmas = tuple(new_pass_std_dev)
        self.motion = tuple(motion_model)
        self.fraction = int(display_points_fraction)
        # DpgSLAM state (dpg_slam.h private members)
        self.pass_number = 0
        self.odom_initialized = False
        self.first_scan_for_pass = True
        self.cum_dist = f32(0.0)
        self.prev_odom = np.zeros(3, f32)               # prev_odom_loc_, prev_odom_angle_
        self.odom_at_last_align = np.zeros(3, f32)      # odom_{loc,angle}_at_last_laser_align_
        self.poses = np.zeros((0, 3), f32)               # dpg_nodes_ estimated positions (float32)
        self.node_pass = np.zeros(0, np.int32)
        self.ranges: list[np.ndarray] = []
        self.geom: list[tuple] = []
        self.clouds: list[np.ndarray] = []
        self.odom_only: list[np.ndarray] = []
        self.current_pass: list[int] = []
        self.factors: list[np.ndarray] = []             # reoptimize's graph (the per-node factors live in the backend)
        self.n_factors = 0                              # graph_->size()
        self._store = None
        self._store_V = 0
        self.last_dpg = None                            # dpg_change_stats of the last executeDPG
        self._loc = None                                # localisation-only mode's state (StartLocalization)
        self.last_track = None                          # the record of the last tracked scan
        self.last_refine = None                         # with field_refine: the refinement's record of that scan
        self._tracked_cov = None                        # the cov of the last accepted refinement (6 doubles) or None

    # ------------------------------------------------------------------ public API
    def ObserveOdometry(self, odom_loc, odom_angle):
        """dpg_slam.cc:515-526."""
        self.odom_initialized = True
        loc = np.asarray(odom_loc, f32)
        d = loc - self.prev_odom[:2]
        self.cum_dist = f32(self.cum_dist + f32(np.sqrt(f32(d[0] * d[0]) + f32(d[1] * d[1]))))
        self.prev_odom = np.array([loc[0], loc[1], f32(odom_angle)], f32)

    def ObserveLaser(self, ranges, range_min, range_max, angle_min, angle_max):
        """dpg_slam.cc:122-140."""
        if self._loc is not None:   # localisation-only mode: track, create nothing
            self._track_laser(np.asarray(ranges, f32), f32(range_max), f32(angle_min), f32(angle_max))
            return
        if not self.odom_initialized:
            return
        if not self._update_pose_graph(np.asarray(ranges, f32), f32(range_max), f32(angle_min), f32(angle_max)):
            return
        if self.pass_number >= 1:
            self.last_dpg = self.executeDPG()

    def incrementPassNumber(self):
        """dpg_slam.cc:25-33."""
        self.pass_number += 1
        self.odom_initialized = False
        self.first_scan_for_pass = True
        self.current_pass = []
        self.reoptimize()

    def GetPose(self):
        """dpg_slam.cc:528-553: the last node's estimate plus the odometry not yet in the graph."""
        if self._loc is not None:   # localisation-only mode: the tracked pose plus the odometry since that track
            return self._tracked_pose()
        loc = self.poses[-1][:2] if len(self.poses) else np.zeros(2, f32)
        ang = self.poses[-1][2] if len(self.poses) else f32(0)
        return self._plus_odometry(loc, ang, self.odom_at_last_align)

    def _plus_odometry(self, loc, ang, odom_ref):
        """(loc, ang) moved by the odometry since odom_ref, as GetPose composes it (dpg_slam.cc:528-553)."""
        un = self.prev_odom[:2] - odom_ref[:2]
        dth = _angle_mod(self.prev_odom[2] - odom_ref[2])   # AngleDiff
        disp = api.transform_point(np.array([un[0], un[1], 0], f32), np.array([0, 0, -odom_ref[2]], f32))
        rot = api.transform_point(np.array([disp[0], disp[1], 0], f32), np.array([0, 0, ang], f32))
        return np.array([loc[0] + rot[0], loc[1] + rot[1]], f32), f32(ang + dth)

    # ------------------------------------------------------------------ localisation-only mode
    def StartLocalization(self, track_params=None, loc_params=None, fmap=None, pose=None, min_response=0.0,
                          icp_refine=True, field_refine=None):
        """Localisation-only mode: from here to StopLocalization every ObserveLaser tracks its scan in a
        frozen map (dpg_fmap_track over track_params' window) and creates no node and no factor; the
        store and the graph are not touched.  fmap None: the current active map is frozen
        (store.freeze(V, poses, loc_params)); else an api.FrozenMap, e.g. a loaded one.  The tracked
        pose starts at `pose` (x, y, theta), or at GetPose() when None.
        Per scan: guess = the tracked pose composed with the odometry since it was set (GetPose's
        arithmetic); r = fmap.track([cloud], [guess])[0], kept in last_track.  With status DPG_LOC_OK
        and score / (255 n_pts) >= min_response the tracked pose becomes r.pose -- or, with icp_refine,
        the pose of one run_icp of the scan at r.pose against the nearest node that was active at the
        freeze, when that ICP converges.  Otherwise it is left alone and dead-reckons on.
        field_refine: a RefineParams (or True for the defaults) replaces the ICP step by the Gauss-Newton
        refinement on the map's own field: (t, f) = fmap.track_refine([cloud], [guess], track_params,
        field_refine), kept in last_track and last_refine; when the track is accepted as above and f's
        status is CONVERGED or MAX_ITERS the tracked pose becomes f.pose, else r.pose.  It needs no node
        cloud, so it works on a loaded map; GetTrackedPoseCovariance() then returns f's covariance."""
        if pose is None and not len(self.poses):
            raise ValueError("StartLocalization: the graph has no node yet and no pose was given")
        V = len(self.poses)
        store = self._dpg_store() if V else None
        if fmap is None:
            fn = getattr(store, "freeze", None)
            if fn is None:
                raise NotImplementedError(f"StartLocalization needs a `freeze(n_nodes, est, params)` method on the backend's "
                                          f"node store; {type(store).__name__} has none")
            fmap, own = fn(V, self.poses, loc_params), True
        else:
            own = False
        if getattr(fmap, "track", None) is None:
            raise NotImplementedError(f"StartLocalization needs a `track(clouds, guesses, params)` method on the map; "
                                      f"{type(fmap).__name__} has none")
        refine = None
        if field_refine is not None and field_refine is not False:
            if getattr(fmap, "track_refine", None) is None:
                raise NotImplementedError(f"StartLocalization(field_refine=...) needs a `track_refine(clouds, guesses, track_params, "
                                          f"refine_params)` method on the map; {type(fmap).__name__} has none")
            refine = _abi.default_refine_params() if field_refine is True else field_refine
        icp = None
        if icp_refine and refine is None:
            icp = getattr(getattr(self.be, "ctx", None), "run_icp", None)
            if icp is None:
                raise NotImplementedError(f"StartLocalization(icp_refine=True) needs a `ctx.run_icp` on the backend; "
                                          f"{type(self.be).__name__} has none")
        nodes = np.arange(V)
        fetch = getattr(store, "fetch", None)
        if V and fetch is not None:
            nodes = np.nonzero(np.asarray(fetch()[2][:V]))[0]
        if pose is None:
            loc, ang = self.GetPose()
            pose = (loc[0], loc[1], ang)
        self.last_track = None
        self.last_refine = None
        self._tracked_cov = None
        self._loc = dict(fmap=fmap, own=own, params=track_params, min_response=float(min_response), icp=icp, refine=refine,
                         nodes=nodes, node_poses=self.poses[nodes].copy(), pose=np.asarray(pose, f32).reshape(3).copy(),
                         odom_ref=self.prev_odom.copy() if self.odom_initialized else None)

    def StopLocalization(self):
        """Leaves the mode and changes nothing else: mapping continues as if the scans delivered in
        between had never arrived.  A map frozen by StartLocalization is closed."""
        if self._loc is not None and self._loc["own"]:
            self._loc["fmap"].close()
        self._loc = None
        self._tracked_cov = None

    def _tracked_pose(self):
        """The tracked pose plus the odometry since it was set."""
        m = self._loc
        if m["odom_ref"] is None:   # no odometry yet: nothing to add
            return m["pose"][:2].copy(), f32(m["pose"][2])
        return self._plus_odometry(m["pose"][:2], m["pose"][2], m["odom_ref"])

    def _track_laser(self, ranges, range_max, angle_min, angle_max):
        m = self._loc
        if m["odom_ref"] is None and self.odom_initialized:
            m["odom_ref"] = self.prev_odom.copy()
        cloud = api.scan_to_cloud(ranges, angle_min, angle_max, range_max, self.laser)
        loc, ang = self._tracked_pose()
        guess = np.array([loc[0], loc[1], ang], f32)
        f = None
        if m["refine"] is not None:
            t, fr = m["fmap"].track_refine([cloud], [guess], m["params"], m["refine"])
            r, f = t[0], fr[0]
            self.last_refine = f
        else:
            r = m["fmap"].track([cloud], [guess], m["params"])[0]
        self.last_track = r
        response = float(r["score"]) / (255.0 * max(int(r["n_pts"]), 1))
        if int(r["status"]) != _abi.DPG_LOC_OK or response < m["min_response"]:
            return                                  # the tracked pose dead-reckons on
        pose = np.array(r["pose"], f32)
        if f is not None:
            self._tracked_cov = None
            if int(f["status"]) in (_abi.DPG_REFINE_CONVERGED, _abi.DPG_REFINE_MAX_ITERS):
                pose = np.array(f["pose"], f32)
                if int(f["cov_ok"]):
                    self._tracked_cov = np.array(f["cov"], np.float64)
        elif m["icp"] is not None and len(m["nodes"]):
            d = m["node_poses"][:, :2].astype(np.float64) - pose[:2].astype(np.float64)
            k = int(np.argmin(d[:, 0] ** 2 + d[:, 1] ** 2))
            t = int(m["nodes"][k])
            ok, z, *_ = m["icp"](api.Node(m["node_poses"][k], self.clouds[t]), api.Node(pose, cloud), self.icp_params)
            if ok:
                pose = api.transform_point(np.array([z[0][0], z[0][1], z[1]], f32), m["node_poses"][k])
        m["pose"] = pose
        m["odom_ref"] = self.prev_odom.copy() if self.odom_initialized else None

    def GetTrackedPoseCovariance(self):
        """The 3x3 covariance (x, y, theta; metres and radians, the map's frame) of the last accepted
        field refinement of localisation-only mode (dpg_refine_result.cov), or None when there is none --
        no field_refine, no accepted refinement yet, the last accepted track fell back to the track's
        pose, or cov_ok is 0.  It is the least-squares curvature estimate in the field's own residual
        units, not a calibrated sensor model."""
        c = self._tracked_cov
        if c is None:
            return None
        return np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]], np.float64)

    def GetPoseCovariance(self, node=None):
        """The 3x3 marginal covariance of a node's pose (default: the latest node), in the pose's own
        tangent frame (dx, dy, dtheta along its body axes) -- isam_->marginalCovariance(key), which
        the reference's DpgSLAM does not expose (its start-up check prints gtsam::Marginals,
        dpg_slam_main.cc:272-279).  Covers the node's graph estimate, not the odometry GetPose adds."""
        V = len(self.poses)
        if V == 0:
            raise ValueError("GetPoseCovariance: the graph has no node yet")
        k = V - 1 if node is None else int(node)
        if not 0 <= k < V:
            raise IndexError(f"GetPoseCovariance: node {node} out of range (the graph has {V} nodes)")
        fn = getattr(self.be, "marginals", None)
        if fn is None:
            raise NotImplementedError(f"GetPoseCovariance needs a `marginals(nodes)` method on the backend; "
                                      f"{type(self.be).__name__} has none")
        return np.asarray(fn([k]), np.float64).reshape(3, 3)

    def GetRelativePoseCovariance(self, i, j):
        """The 3x3 covariance of the relative pose X_i^-1 X_j between two nodes of the graph, in
        that relative pose's own tangent frame -- what a covariance gate of a loop-closure candidate
        (i, j) reads before an ICP alignment is spent on it; the nodes need not share a factor
        (gtsam::Marginals::jointMarginalCovariance and the Between Jacobians).  Zero for i == j."""
        V = len(self.poses)
        if V == 0:
            raise ValueError("GetRelativePoseCovariance: the graph has no node yet")
        i, j = int(i), int(j)
        for k in (i, j):
            if not 0 <= k < V:
                raise IndexError(f"GetRelativePoseCovariance: node {k} out of range (the graph has {V} nodes)")
        fn = getattr(self.be, "relative_covariances", None)
        if fn is None:
            raise NotImplementedError(f"GetRelativePoseCovariance needs a `relative_covariances(pairs)` method on "
                                      f"the backend; {type(self.be).__name__} has none")
        return np.asarray(fn([(i, j)]), np.float64).reshape(3, 3)

    def GetMap(self):
        """dpg_slam.cc:555-575."""
        if not len(self.poses):
            return np.zeros((0, 2), f32)
        return self.be.get_map(self._clouds, self.poses, self.fraction, self.icp_params.downsample_icp_points_ratio)

    def GetActiveAndDynamicMapPoints(self):
        """getActiveAndDynamicMapPoints (dpg_slam.cc:832-863) over the current node state."""
        return self._dpg_store().active_dynamic_points(len(self.poses), self.poses)

    def GetOccupancyGrid(self, resolution=None):
        """The occupancy grid of the active pose graph over the current node state -- the fields of a
        nav_msgs/OccupancyGrid: dict of `resolution`, `origin` (x, y), `width`, `height` and `data`
        (int8 [height, width]: -1 unknown, 0..100 occupancy).  resolution None: the
        change detection's occ_grid_resolution.  The reference only hands back point lists."""
        V = len(self.poses)
        if V == 0:
            raise ValueError("GetOccupancyGrid: the graph has no node yet")
        if resolution is not None and not float(resolution) > 0.0:
            raise ValueError(f"GetOccupancyGrid: resolution must be positive, got {resolution!r}")
        store = self._dpg_store()
        fn = getattr(store, "occupancy_grid", None)
        if fn is None:
            raise NotImplementedError(f"GetOccupancyGrid needs an `occupancy_grid(n_nodes, est, params)` method on the "
                                      f"backend's node store; {type(store).__name__} has none")
        p = _abi.default_grid_params()
        if resolution is not None:
            p.resolution = float(resolution)
        return fn(V, self.poses, p)

    def Localize(self, ranges, range_max, angle_min, angle_max, guess=None, params=None):
        """The pose of a scan in the active map over the current node state (dpg_map_localize): a
        LOC_RESULT_DTYPE record, pose in the map frame (the frame of GetPose).  guess None: the whole
        map around its centre; else (x, y, theta) with the params' window around it."""
        V = len(self.poses)
        if V == 0:
            raise ValueError("Localize: the graph has no node yet")
        store = self._dpg_store()
        fn = getattr(store, "localize", None)
        if fn is None:
            raise NotImplementedError(f"Localize needs a `localize(n_nodes, est, cloud, guess, params, window)` method on "
                                      f"the backend's node store; {type(store).__name__} has none")
        cloud = api.scan_to_cloud(np.asarray(ranges, f32), f32(angle_min), f32(angle_max), f32(range_max), self.laser)
        if guess is None:
            return fn(V, self.poses, cloud, (0.0, 0.0, 0.0), params, "map")
        return fn(V, self.poses, cloud, guess, params, None)

    def executeDPG(self):
        """dpg_slam.cc:865-886 (dpg_execute_dpg on the node store)."""
        return self._dpg_store().execute_dpg(len(self.poses), len(self.current_pass), self.poses)

    def reoptimize(self):
        """dpg_slam.cc:35-120: a fresh graph -- per node the pass prior or the odometry Between, the
        successive alignment (always a factor) and every loop-closure candidate (a factor when
        converged), all aligned in one batch from the current estimates -- then one update of a new
        graph from the current estimates."""
        V = len(self.poses)
        if V == 0:
            return
        t0 = time.perf_counter()
        ms_verify = None
        est = self.poses.copy()
        passes = self.node_pass
        lc = self.be.candidates(est, passes, float(self.within), float(self.across))
        t1 = time.perf_counter()
        succ = np.stack([np.arange(V - 1), np.arange(1, V)], 1).astype(np.int32)
        edges = np.concatenate([succ, np.asarray(lc, np.int32).reshape(-1, 2)], 0)
        res = None
        if len(edges) and self.prematch_params is not None:
            res = self._icp_batch_prematched(edges, len(succ), est)
        elif len(edges):
            res = self.be.icp_batch(self._clouds, edges, est, self.icp_params)
        t2 = time.perf_counter()
        # per node, in node order: the pass's prior on its first node, else the odometry Between
        # from the previous node (dpg_slam.cc:41-75) -- built for all nodes at once
        pv = np.asarray(passes)
        start = np.ones(V, bool)
        start[1:] = pv[1:] != pv[:-1]
        keep_n = start | bool(self.odometry_constraints)
        Fn = np.zeros(V, FACTOR_DTYPE)
        Fn[start] = api.prior_factors(np.nonzero(start)[0], sigmas=self.prior_sigmas)
        for n, pose in self.pass_start_pose.items():   # the passes that started from a localised pose
            Fn[n] = api.prior_factor(n, pose=pose, sigmas=self.prior_sigmas)
        odo = np.nonzero(~start)[0] if self.odometry_constraints else np.zeros(0, np.int64)
        if len(odo):
            Fn[odo] = api.odometry_factors(np.asarray(self.odom_only, f32), odo - 1, odo, self.motion)
        F = [Fn[keep_n]]
        if len(edges):
            # addObservationConstraint per aligned pair (dpg_icp_factor, vectorised): the successive
            # pairs always, a loop closure when its alignment converged (dpg_slam.cc:85-104)
            keep = np.ones(len(edges), bool)
            keep[len(succ):] = (res["converged"][len(succ):] != 0) & (res["status"][len(succ):] == _abi.DPG_ICP_OK)
            if self.verify_params is not None:
                tv = time.perf_counter()
                self._verify_closures(edges, len(succ), res, keep)
                ms_verify = (time.perf_counter() - tv) * 1e3
            Fi = np.zeros(int(keep.sum()), FACTOR_DTYPE)
            Fi["kind"] = _abi.DPG_FACTOR_BETWEEN
            Fi["i"], Fi["j"] = edges[keep, 0], edges[keep, 1]
            Fi["z"] = res["z"][keep].astype(np.float64)
            p = self.icp_params
            Fi["info"] = [1.0 / float(f32(p.laser_x_variance)), 1.0 / float(f32(p.laser_y_variance)),
                          1.0 / float(f32(p.laser_theta_variance))]
            F.append(Fi)
        F = np.concatenate([np.asarray(f, FACTOR_DTYPE).reshape(-1) for f in F])
        self.factors = F
        self.n_factors = len(F)
        t3 = time.perf_counter()
        X = self.be.rebuild_graph(est.astype(np.float64), F)
        self.poses = np.asarray(X, f32).reshape(-1, 3)
        # the sweep's phases (ms): candidate search, the batched ICP, the factor list, the new graph's update
        self.last_sweep_ms = {"candidates": (t1 - t0) * 1e3, "icp": (t2 - t1) * 1e3,
                              "factors": (t3 - t2) * 1e3 - (ms_verify or 0.0),
                              "update": (time.perf_counter() - t3) * 1e3, "edges": int(len(edges))}
        if ms_verify is not None:   # with loop_closure_verify: the check of the converged loop closures
            self.last_sweep_ms["verify"] = ms_verify
        st = getattr(self.be, "last_rebuild", None)
        if st is not None:
            self.last_sweep_ms.update(update_symbolic=st.ms_symbolic, update_numeric=st.ms_numeric,
                                      gn_iterations=int(st.gn_iterations))

    # ------------------------------------------------------------------ internals
    def _icp_batch_prematched(self, edges, n_succ, est):
        """The sweep's alignments with loop_closure_prematch on: every edge's guess is
        dpg_icp_guess's, except the loop-closure candidates (edges[n_succ:]) the matcher answered
        with a response of at least prematch_min_response, which start from its refined guess."""
        for name in ("prematch", "icp_batch_guess"):
            if getattr(self.be, name, None) is None:
                raise NotImplementedError(f"loop_closure_prematch needs a `{name}` method on the backend; "
                                          f"{type(self.be).__name__} has none")
        guesses = np.stack([api.icp_guess(est[s], est[t]) for t, s in edges]).astype(f32)
        self.last_prematch = None
        if len(edges) > n_succ:
            m = self.be.prematch(self._clouds, edges[n_succ:], est, self.prematch_params,
                                 self.icp_params.downsample_icp_points_ratio)
            response = m["score"] / (255.0 * np.maximum(m["n_src"], 1))
            take = response >= self.prematch_min_response
            guesses[n_succ:][take] = m["guess"][take]
            self.last_prematch = m
        return self.be.icp_batch_guess(self._clouds, edges, guesses, len(est), self.icp_params)

    def _verify_closures(self, edges, n_succ, res, keep):
        """With loop_closure_verify on: clears keep[] of the converged loop-closure candidates
        (edges[n_succ:]) that the free-space check under their ICP transform does not accept."""
        fn = getattr(self.be, "verify", None)
        if fn is None:
            raise NotImplementedError(f"loop_closure_verify needs a `verify` method on the backend; "
                                      f"{type(self.be).__name__} has none")
        idx = np.nonzero(keep[n_succ:])[0] + n_succ
        ve = np.ascontiguousarray(edges[idx], np.int32).reshape(-1, 2)
        self.last_verify = (np.zeros(0, _abi.VERIFY_RESULT_DTYPE), ve)
        if not len(idx):
            return
        T = np.ascontiguousarray(res["T"][idx], f32).reshape(-1, 6)
        rec = fn(self._clouds, ve, T, self.verify_params, self.icp_params.downsample_icp_points_ratio)
        keep[idx] = api.verify_accept(rec, self.verify_max_free, self.verify_min_support)
        self.last_verify = (rec, ve)

    def _odometry_factor(self, prev, cur, i, j):
        f = api.odometry_factor(prev, cur, i, j, self.motion)
        return np.frombuffer(bytes(f), FACTOR_DTYPE).copy()

    def _clouds(self):
        offs = np.zeros(len(self.clouds) + 1, np.int64)
        offs[1:] = np.cumsum([len(c) for c in self.clouds])
        pts = np.concatenate(self.clouds) if self.clouds else np.zeros((0, 2), f32)
        return np.ascontiguousarray(pts, f32), offs

    def _create_node(self, ranges, range_max, angle_min, angle_max, pose):
        """createNode (dpg_slam.cc:488-513): the base_link cloud of the scan, MAX_RANGE dropped."""
        cloud = api.scan_to_cloud(ranges, angle_min, angle_max, range_max, self.laser)
        self.poses = np.concatenate([self.poses, np.asarray(pose, f32).reshape(1, 3)])
        self.node_pass = np.append(self.node_pass, np.int32(self.pass_number))
        self.ranges.append(ranges.copy())
        self.geom.append((angle_min, angle_max, range_max))
        self.clouds.append(np.ascontiguousarray(cloud, f32))
        return len(self.poses) - 1

    def _should_process_laser(self):
        """dpg_slam.cc:577-589."""
        angle_diff = f32(abs(_angle_mod(self.prev_odom[2] - self.odom_at_last_align[2])))
        if self.cum_dist > self.min_dist or angle_diff > self.min_angle:
            self.cum_dist = f32(0.0)
            return True
        return False

    def _update_pose_graph(self, ranges, range_max, angle_min, angle_max):
        """dpg_slam.cc:160-253."""
        if self.first_scan_for_pass:
            self.first_scan_for_pass = False
            start = self._new_pass_start(ranges, range_max, angle_min, angle_max)
            if start is None:
                n = self._create_node(ranges, range_max, angle_min, angle_max, (0.0, 0.0, 0.0))
                extra = api.prior_factor(n, sigmas=self.prior_sigmas)
            else:
                n = self._create_node(ranges, range_max, angle_min, angle_max, start)
                extra = api.prior_factor(n, pose=start, sigmas=self.prior_sigmas)
                self.pass_start_pose[n] = start
            self.odom_only.append(self.prev_odom.copy())
            self.odom_at_last_align = self.prev_odom.copy()
            if self.pass_number == 0:   # the first node: the prior only, then optimizeGraph (:189-202)
                self._add_node(n, extra, aligned=False)
                return False
            self._add_node(n, extra)
            return True
        if not self._should_process_laser():
            return False
        rel = api.inverse_transform_point(self.prev_odom, self.odom_at_last_align)   # displacement since the last node
        pose = api.transform_point(rel, self.poses[-1])                                # createRelativePositionedNode
        n = self._create_node(ranges, range_max, angle_min, angle_max, pose)
        extra = self._odometry_factor(self.odom_at_last_align, self.prev_odom, n - 1, n) if self.odometry_constraints \
            else np.zeros(0, FACTOR_DTYPE)
        self.odom_only.append(self.prev_odom.copy())
        self.odom_at_last_align = self.prev_odom.copy()
        self._add_node(n, extra)
        return True

    def _new_pass_start(self, ranges, range_max, angle_min, angle_max):
        """The localised pose (x, y, theta) a pass >= 1 starts from, or None for the reference's origin."""
        if self.new_pass_start is None or self.pass_number == 0 or not len(self.poses):
            return None
        r = self.Localize(ranges, range_max, angle_min, angle_max, params=self.new_pass_start)
        self.last_localization = r
        response = float(r["score"]) / (255.0 * max(int(r["n_pts"]), 1))
        if int(r["status"]) not in (_abi.DPG_LOC_OK, _abi.DPG_LOC_UNPROVEN) or response < self.localize_min_response:
            return None
        return tuple(float(v) for v in r["pose"])

    def _add_node(self, n, extra, aligned=True):
        """updatePoseGraphObsConstraints (dpg_slam.cc:255-314) + optimizeGraph: the backend aligns the
        new node n with the preceding one and the preceding one with every earlier node within the
        distance rule (one batch), adds the factors and updates the graph."""
        extra = np.asarray(extra, FACTOR_DTYPE).reshape(-1)
        n_icp, X = self.be.add_node(self.clouds[n], self.node_pass, self.poses[n], extra,
                                    self.icp_params, self._reopt_params(), aligned and self.non_successive)
        self.n_factors += len(extra) + n_icp
        self.current_pass.append(n)
        self.poses = np.asarray(X, f32).reshape(-1, 3)

    def _reopt_params(self):
        rp = _abi.default_reopt_params()
        rp.max_node_dist_within_pass = float(self.within)
        rp.max_node_dist_across_passes = float(self.across)
        return rp

    def _dpg_store(self):
        """The node store over every node so far: created once, then the new nodes' scans are
        appended (dpg_dpg_append keeps the labels, sectors and activity of the others)."""
        V = len(self.poses)
        if self._store_V != V:
            rs = self.ranges[self._store_V:]
            offs = np.zeros(len(rs) + 1, np.int64)
            offs[1:] = np.cumsum([len(r) for r in rs])
            rng = np.ascontiguousarray(np.concatenate(rs), f32)
            geom = np.asarray(self.geom[self._store_V:], f32)
            if self._store is None:
                self._store = self.be.store(rng, geom, offs, self.change_params)
            else:
                self._store.append(rng, geom, offs)
            self._store_V = V
        return self._store
