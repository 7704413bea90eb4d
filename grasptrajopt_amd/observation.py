"""Observation — what the robot observed, resident on the GPU, and the collision checks against it (gto_observation_*,
gto_check_plans: include/gto_solver.h).

The reference keeps its observation alive as an object (``DepthPointCloud`` owns its KD-tree,
mesh_to_sdf/depth_point_cloud.py:25) and asks it many times: the grasp collision filter of the planning driver
(examples/pybullet_gto_planning.py:203-221) and the plan collision statistic of the offline evaluator
(examples/pybullet_evaluate_plans.py:219-233).  An ``Observation`` is built once from a ``DepthPointCloud`` or a
``SurfacePointCloud`` (their ``observation()``), owns its device memory until ``close()``, and answers

    sdf(points)                       get_sdf / inside at world points (the bits of the stand-alone entry points)
    check_posed(points, poses)        per pose, how many of the placed points are inside (the grasp filter)
    check_plans(handle, plans, base)  per plan and waypoint, how many robot surface points are inside (the plan statistic)
    check_held_paths(handle, paths, held_points, ...)  per path and column, how many points of the object the robot holds
                                      are inside (the motion after the grasp)

with only the counts coming back to the host.  "Inside" is ``get_sdf < 0`` of the reference except at a query that
coincides with a cloud point (include/gto_solver.h).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import GTOError

_pd, _pf, _pi, _pu8 = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


class Observation:
    """Owns one gto_observation (one HIP device)."""

    def __init__(self, ptr, lib, kind: str, device: int):
        self._o, self._lib, self.kind, self.device = ptr, lib, kind, device

    @classmethod
    def from_depth(cls, depth, intrinsic_matrix, camera_pose, target_mask=None, threshold=1.5, device=0, Kinv=None, cam_inv=None):
        """gto_observation_from_depth; Kinv / cam_inv default to numpy.linalg.inv of the matrices, as the reference inverts."""
        lib = _capi.load_library()
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        if depth.ndim != 2:
            raise GTOError(f"Observation.from_depth: the depth image must be (H, W), got {depth.shape}")
        K = np.ascontiguousarray(intrinsic_matrix, dtype=np.float64).reshape(3, 3)
        cam = np.ascontiguousarray(camera_pose, dtype=np.float64).reshape(4, 4)
        Kinv = np.ascontiguousarray(np.linalg.inv(K) if Kinv is None else Kinv, dtype=np.float64)
        cinv = np.ascontiguousarray(np.linalg.inv(cam) if cam_inv is None else cam_inv, dtype=np.float64)
        mask = None if target_mask is None else np.ascontiguousarray(target_mask, dtype=np.uint8)
        if mask is not None and mask.shape != depth.shape:
            raise GTOError("Observation.from_depth: target_mask must have the shape of depth")
        o = C.c_void_p()
        rc = lib.gto_observation_from_depth(int(device), _p(depth, _pf), depth.shape[0], depth.shape[1], _p(K, _pd), _p(Kinv, _pd), _p(cam, _pd),
                                            _p(cinv, _pd), _p(mask, _pu8), float(threshold), C.byref(o))
        if rc != 0:
            raise GTOError(f"gto_observation_from_depth failed ({rc}): {lib.gto_last_error(None).decode()}")
        return cls(o, lib, "depth", int(device))

    @classmethod
    def from_cloud(cls, points, normals, sample_count=11, device=0):
        """gto_observation_from_cloud: surface samples and their normals, the vote of the ``sample_count`` nearest."""
        lib = _capi.load_library()
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
        if pts.shape != nrm.shape:
            raise GTOError("Observation.from_cloud: points and normals must have the same shape")
        o = C.c_void_p()
        rc = lib.gto_observation_from_cloud(int(device), _p(pts, _pd), _p(nrm, _pd), pts.shape[0], int(sample_count), C.byref(o))
        if rc != 0:
            raise GTOError(f"gto_observation_from_cloud failed ({rc}): {lib.gto_last_error(None).decode()}")
        return cls(o, lib, "cloud", int(device))

    # ------------------------------------------------------------------ lifetime
    def _ptr(self):
        if not getattr(self, "_o", None):
            raise GTOError("this Observation is closed: its device memory was released by close()")
        return self._o

    @property
    def closed(self) -> bool:
        return not getattr(self, "_o", None)

    def close(self):
        if getattr(self, "_o", None):
            self._lib.gto_observation_destroy(self._o)
            self._o = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise GTOError(f"{what} failed ({rc}): {self._lib.gto_last_error(None).decode()}")

    # ------------------------------------------------------------------ queries
    def sdf(self, query_points):
        """(sdf float32 (nq,), inside bool (nq,)) at world points (nq, 3): get_sdf and ~is_outside (depth) or the vote (cloud)."""
        o = self._ptr()
        q = np.ascontiguousarray(query_points, dtype=np.float64).reshape(-1, 3)
        sdf, inside = np.empty(q.shape[0], dtype=np.float32), np.empty(q.shape[0], dtype=np.uint8)
        self._check(self._lib.gto_observation_sdf(o, _p(q, _pd), q.shape[0], _p(sdf, _pf), _p(inside, _pu8)), "gto_observation_sdf")
        return sdf, inside.astype(bool)

    def check_posed(self, points, poses):
        """int32 (n,): how many of points (P, 3), placed at each of poses (n, 4, 4), are inside; -1 for a non-finite pose."""
        o = self._ptr()
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        RT = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 16)
        count = np.empty(RT.shape[0], dtype=np.int32)
        self._check(self._lib.gto_observation_check_posed(o, _p(pts, _pd), pts.shape[0], _p(RT, _pd), RT.shape[0], _p(count, _pi)),
                    "gto_observation_check_posed")
        return count

    def check_plans(self, handle, plans, base_pos=(0.0, 0.0, 0.0)):
        """int32 (B, T): SolverHandle.check_plans of ``handle`` against this observation."""
        return handle.check_plans(self, plans, base_pos)

    def check_held_paths(self, robot_or_handle, paths, held_points, n_held=None, attach=None, attach_col=None, object_pose=None,
                         labels=None, held_label=None, base_pos=(0.0, 0.0, 0.0), link_ee=None, link_gripper=None):
        """int32 (B, Tp): SolverHandle.check_held_paths against this observation -- per path (B, ndof, Tp) and column, how many
        of the held object's points, carried rigidly with link_ee from the configuration of the grasp, are inside.
        held_points: a list of per-plan (n_i, 3) arrays, or a padded array (B, P_max, 3) with n_held (B,).
        robot_or_handle: a ``SolverHandle``, or a robot model (``GTORobotModel``) together with link_ee / link_gripper, whose
        cached handle is used.  The other arguments: ``SolverHandle.check_held_paths``."""
        handle = robot_or_handle
        if not hasattr(handle, "check_held_paths"):
            if link_ee is None:
                raise GTOError("Observation.check_held_paths: a robot model needs link_ee (and link_gripper, default: link_ee)")
            handle = robot_or_handle.solver_handle(link_ee, link_ee if link_gripper is None else link_gripper, _capi.default_opts(),
                                                   role="retrieve")
        return handle.check_held_paths(self, paths, held_points, n_held=n_held, attach=attach, attach_col=attach_col,
                                       object_pose=object_pose, labels=labels, held_label=held_label, base_pos=base_pos)


def as_observation(cloud_or_obs) -> Observation:
    """An Observation, or the cached one of a DepthPointCloud / SurfacePointCloud."""
    if isinstance(cloud_or_obs, Observation):
        return cloud_or_obs
    if hasattr(cloud_or_obs, "observation"):
        return cloud_or_obs.observation()
    raise GTOError(f"expected an Observation, a DepthPointCloud or a SurfacePointCloud, got {type(cloud_or_obs).__name__}")
