"""Host-side helpers of the GTO layer (gto/utils.py in the reference)."""
from __future__ import annotations

import os

import numpy as np
import yaml

from .synthetic import interpolate_waypoints as _interp2


def get_root_dir() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def load_yaml(file_path):
    """gto/utils.py:15-21."""
    if isinstance(file_path, str):
        with open(file_path) as fh:
            return yaml.load(fh, Loader=yaml.Loader)
    return file_path


def rotZ(rotz: float) -> np.ndarray:
    """gto/utils.py:24-33."""
    c, s = np.cos(rotz), np.sin(rotz)
    return np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])


def mat2quat(M) -> np.ndarray:
    """transforms3d.quaternions.mat2quat, which the reference's IK solvers import (gto/ik_solver_quaternion.py:16):
    (w, x, y, z) of a rotation matrix as the eigenvector of the largest eigenvalue of Bar-Itzhack's symmetric 4x4
    matrix (robust to a not quite orthonormal input), with w >= 0."""
    Qxx, Qyx, Qzx, Qxy, Qyy, Qzy, Qxz, Qyz, Qzz = np.asarray(M, dtype=np.float64)[:3, :3].flat
    K = np.array([[Qxx - Qyy - Qzz, 0, 0, 0],
                  [Qyx + Qxy, Qyy - Qxx - Qzz, 0, 0],
                  [Qzx + Qxz, Qzy + Qyz, Qzz - Qxx - Qyy, 0],
                  [Qyz - Qzy, Qzx - Qxz, Qxy - Qyx, Qxx + Qyy + Qzz]]) / 3.0
    vals, vecs = np.linalg.eigh(K)  # (the lower triangle)
    q = vecs[[3, 0, 1, 2], np.argmax(vals)]
    if q[0] < 0:
        q *= -1
    return q


def quat2rpy(x, y, z, w) -> np.ndarray:
    """optas Quaternion(x, y, z, w).getrpy() (optas/spatialmath.py:410-430): roll, pitch, yaw; pitch is +pi/2 whenever
    |sin(pitch)| >= 1, -1 included (the reference's rule, kept)."""
    roll = np.arctan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + y * y))
    sinp = 2.0 * (w * y - z * x)
    pitch = np.pi / 2.0 if abs(sinp) >= 1.0 else np.arcsin(sinp)
    yaw = np.arctan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))
    return np.array([roll, pitch, yaw])


def ik_goal_quaternion(RT) -> np.ndarray:
    """tf_goal of gto/ik_solver_quaternion.py:81-84: x y z qx qy qz qw of a 4x4 goal pose."""
    RT = np.asarray(RT, dtype=np.float64)
    w, x, y, z = mat2quat(RT[:3, :3])
    return np.array([RT[0, 3], RT[1, 3], RT[2, 3], x, y, z, w])


def ik_goal_rpy(RT) -> np.ndarray:
    """tf_goal of gto/ik_solver_rpy.py:84-89: x y z roll pitch yaw of a 4x4 goal pose."""
    RT = np.asarray(RT, dtype=np.float64)
    w, x, y, z = mat2quat(RT[:3, :3])
    return np.concatenate([RT[:3, 3], quat2rpy(x, y, z, w)])


def interpolate_waypoints(waypoints, n: int, m: int, mode: str = "cubic") -> np.ndarray:
    """gto/utils.py:63-82: clamped cubic through the waypoints sampled at linspace(0,1,n+2)[1:-1]
    (endpoints excluded).  The planner only ever passes two waypoints (gto/gto_planner.py:155,203),
    for which the clamped spline is the closed-form Hermite cubic; more waypoints go through scipy."""
    w = np.asarray(waypoints, dtype=np.float64)
    if mode == "cubic" and w.shape[0] == 2:
        return _interp2(w, n, m)
    from scipy import interpolate
    data = np.zeros([n, m])
    x = np.linspace(0, 1, w.shape[0])
    t = np.linspace(0, 1, n + 2)
    for i in range(w.shape[1]):
        f = (interpolate.interp1d(x, w[:, i], "linear") if mode == "linear"
             else interpolate.CubicSpline(x, w[:, i], bc_type="clamped"))
        data[:, i] = f(t[1:-1])
    return data


def plan_in_collision(robot, depth_pc, plan, base_position=(0.0, 0.0, 0.0), max_points: int = 5, is_mobile: bool = False):
    """The collision statistic of the reference's offline evaluator (examples/pybullet_evaluate_plans.py:
    219-233): a plan collides if at some waypoint more than ``max_points`` robot surface points have a
    negative signed distance to the observed scene.  All waypoints go to the GPU in two calls (FK of the
    surface points, then DepthPointCloud.get_sdf) instead of a Python loop with a KD-tree query per waypoint.
    Returns (in_collision, first_colliding_waypoint or -1, points_in_collision (T,))."""
    plan = np.asarray(plan, dtype=np.float64)
    T = plan.shape[1]
    h = robot._util_handle()
    xyz, _, _, _ = h.eval_points(0, plan.T, [0, 0, 0], want_field=False)  # (T, P, 3), robot-base frame
    if not is_mobile:
        xyz = xyz + np.asarray(base_position, dtype=np.float64).reshape(1, 1, 3)
    sdf = depth_pc.get_sdf(xyz.reshape(-1, 3)).reshape(T, -1)
    count = (sdf < 0).sum(axis=1)
    hit = np.nonzero(count > max_points)[0]
    return bool(hit.size), int(hit[0]) if hit.size else -1, count


def grasp_collision_ratio(gripper_model, depth_pc, RT_grasps, q_gripper, RT_offset=None):
    """The grasp collision filter of the planning driver (examples/pybullet_gto_planning.py:203-219,
    examples/pybullet_gto_planning_mobile.py:307-322): for every candidate grasp pose the open gripper's
    surface points are placed at ``RT_grasp @ RT_offset`` and the fraction with a negative signed distance to
    the observed obstacles is returned (the driver rejects ratios above 0.01).  The gripper's points are
    computed once and all n x P placed points go to the GPU in ONE DepthPointCloud.get_sdf call instead of
    one FK + one KD-tree query per grasp.  Returns ratio (n,) float64."""
    RT = np.asarray(RT_grasps, dtype=np.float64).reshape(-1, 4, 4)
    if RT_offset is not None:
        RT = RT @ np.asarray(RT_offset, dtype=np.float64)
    pts, _ = gripper_model.compute_fk_surface_points(q_gripper)  # gripper frame, (P, 3)
    world = np.einsum("nij,pj->npi", RT[:, :3, :3], pts) + RT[:, None, :3, 3]
    sdf = np.asarray(depth_pc.get_sdf(world.reshape(-1, 3))).reshape(RT.shape[0], -1)
    return (sdf < 0).sum(axis=1) / sdf.shape[1]


def filter_grasps(gripper_model, depth_pc, RT_grasps, q_gripper, RT_offset=None, threshold: float = 0.01):
    """in_collision (n,) int32 exactly as the driver builds it: ratio > threshold."""
    return (grasp_collision_ratio(gripper_model, depth_pc, RT_grasps, q_gripper, RT_offset) > threshold).astype(np.int32)


def plans_in_collision(robot, cloud_or_obs, plans, base_position=(0.0, 0.0, 0.0), max_points: int = 5, is_mobile: bool = False):
    """plan_in_collision for a batch, against a resident observation (observation.Observation, or the cached one of a
    DepthPointCloud / SurfacePointCloud): plans (B, ndof, T) or one plan (ndof, T); base_position (3,) or one per plan (B, 3),
    ignored with is_mobile (examples/pybullet_evaluate_plans.py:224-227).  Kinematics, visibility test (or k-nearest vote)
    and counting run on the GPU (gto_check_plans); only the counts come back.  Returns (in_collision (B,) bool,
    first colliding waypoint (B,) or -1, points in collision (B, T) int32; -1 marks a waypoint with a non-finite entry)."""
    from .observation import as_observation
    plans = np.asarray(plans, dtype=np.float64)
    if plans.ndim == 2:
        plans = plans[None]
    base = np.zeros(3) if is_mobile else np.asarray(base_position, dtype=np.float64)
    counts = _retime_handle(robot, plans.shape[-1]).check_plans(as_observation(cloud_or_obs), plans, base)
    over = counts > max_points
    hit = over.any(axis=1)
    return hit, np.where(hit, over.argmax(axis=1), -1), counts


def grasp_collision_counts(gripper_model, cloud_or_obs, RT_grasps, q_gripper, RT_offset=None):
    """grasp_collision_ratio against a resident observation: the open gripper's surface points are placed at every
    ``RT_grasp @ RT_offset`` and tested on the GPU (gto_observation_check_posed); only the counts come back.  Returns
    (counts (n,) int32, P): counts / P is grasp_collision_ratio's value, and the driver rejects counts / P > 0.01."""
    from .observation import as_observation
    RT = np.asarray(RT_grasps, dtype=np.float64).reshape(-1, 4, 4)
    if RT_offset is not None:
        RT = RT @ np.asarray(RT_offset, dtype=np.float64)
    pts, _ = gripper_model.compute_fk_surface_points(q_gripper)  # gripper frame, (P, 3)
    return as_observation(cloud_or_obs).check_posed(pts, RT), int(pts.shape[0])


def pose_product(A, B) -> np.ndarray:
    """A @ B for 4x4 matrices (leading axes broadcast) as gto_filter_grasps_device forms it: the full product, entry (r, c) =
    ((A_r0 B_0c + A_r1 B_1c) + A_r2 B_2c) + A_r3 B_3c, written with elementwise operations, which numpy does not fuse
    (numpy.matmul goes through BLAS and promises no bits)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    a = lambda k: A[..., :, k, None]
    b = lambda k: B[..., None, k, :]
    return ((a(0) * b(0) + a(1) * b(1)) + a(2) * b(2)) + a(3) * b(3)


def filter_grasp_sets(observations, gripper_points, object_poses, grasps, n_grasps, check_offset, ik_offset=None,
                      world_to_base=None, base_position=None, max_ratio: float = 0.01):
    """The driver's checking stage (examples/pybullet_gto_planning.py:203-236, examples/pybullet_gto_planning_mobile.py:
    313-343) for B objects on the host, object by object: what gto_filter_grasps_device computes on the stream
    (include/gto_solver.h), in numpy on top of ``Observation.check_posed``.

    observations: one entry for all objects or one per object (an Observation, a DepthPointCloud or a SurfacePointCloud);
    gripper_points (P, 3); object_poses (B, 4, 4); grasps (B, n_max, 4, 4) in the object frame; n_grasps (B,), read as
    clamped to [1, n_max]; check_offset (4, 4); ik_offset (4, 4) or None; world_to_base (B, 4, 4) or None; base_position
    (3,), (B, 3) or None.  Returns a dict: counts (B, n_max) int32 (-1: a non-finite row, and the rows beyond n_grasps),
    keep (B, n_max) bool, kept_rows (B, n_max) int32 (-1 beyond the kept ones), n_kept (B,), n_grasps (B,) = max(n_kept, 1),
    plan_goals and ik_goals (B, n_max, 4, 4): the kept rows' goals in their order, zeros behind them; an object without a
    kept row holds row 0's goals at position 0."""
    from .observation import as_observation
    O = np.asarray(object_poses, dtype=np.float64).reshape(-1, 4, 4)
    B = O.shape[0]
    R = np.asarray(grasps, dtype=np.float64)
    n_max = R.shape[1]
    R = R.reshape(B, n_max, 4, 4)
    pts = np.asarray(gripper_points, dtype=np.float64).reshape(-1, 3)
    P = pts.shape[0]
    one = not isinstance(observations, (list, tuple))
    obs = [as_observation(o) for o in ([observations] * B if one else observations)]
    n_in = np.clip(np.broadcast_to(np.asarray(n_grasps, dtype=np.int64), (B,)), 1, n_max)
    W = None if world_to_base is None else np.asarray(world_to_base, dtype=np.float64).reshape(B, 4, 4)
    base = None if base_position is None else np.broadcast_to(np.asarray(base_position, dtype=np.float64).reshape(-1, 3), (B, 3))
    Sc = np.asarray(check_offset, dtype=np.float64).reshape(4, 4)
    Si = None if ik_offset is None else np.asarray(ik_offset, dtype=np.float64).reshape(4, 4)
    out = dict(counts=np.full((B, n_max), -1, np.int32), keep=np.zeros((B, n_max), bool), kept_rows=np.full((B, n_max), -1, np.int32),
               n_kept=np.zeros(B, np.int32), n_grasps=np.ones(B, np.int32), plan_goals=np.zeros((B, n_max, 4, 4)),
               ik_goals=np.zeros((B, n_max, 4, 4)))
    for b in range(B):
        n = int(n_in[b])
        with np.errstate(all="ignore"):
            G = pose_product(O[b], R[b, :n])
            if W is not None:
                G = pose_product(W[b], G)
            Cm = pose_product(G, Sc)
            A = G.copy()
            if base is not None:
                A[:, :3, 3] = G[:, :3, 3] - base[b]
            ik = A if Si is None else pose_product(A, Si)
        bad = ~(np.isfinite(O[b]).all() & np.isfinite(R[b, :n]).all(axis=(1, 2)) & np.isfinite(Cm).all(axis=(1, 2)))
        if W is not None:
            bad |= ~np.isfinite(W[b]).all()
        counts = np.where(bad, -1, obs[b].check_posed(pts, Cm)).astype(np.int32)
        keep = (counts >= 0) & (counts.astype(np.float64) / float(P) <= max_ratio)
        rows = np.flatnonzero(keep)
        out["counts"][b, :n], out["keep"][b, :n] = counts, keep
        out["n_kept"][b], out["n_grasps"][b] = len(rows), max(len(rows), 1)
        out["kept_rows"][b, :len(rows)] = rows
        take = rows if len(rows) else np.array([0])
        out["plan_goals"][b, :len(take)], out["ik_goals"][b, :len(take)] = A[take], ik[take]
    return out


def _retime_handle(robot, T: int):
    """The robot's utility handle for horizon T (retiming and the plan checks only read the handle's T and the robot)."""
    from . import _capi
    o = _capi.default_opts()
    o.T = int(T)
    o.standoff_offset = max(int(o.standoff_offset), 2 - int(T))  # any valid standoff waypoint: retiming does not use it
    ln = robot.desc.link_names[-1]
    return robot.solver_handle(ln, ln, o, role="util")


def _torque_request(robot, tau_max, payload, B, link_ee):
    """The checked (tau_max, payload, link_ee) of a profile="torque" request, before any handle is made."""
    from . import _capi
    tm = _capi.retime_torque_limits(robot.desc, tau_max)
    _capi.payload_arrays(payload, B)
    if payload is not None and link_ee is None:
        raise ValueError("retime: a payload needs link_ee, the link that carries it")
    return tm, payload, robot.desc.link_names[-1] if link_ee is None else link_ee


def _torque_handle(robot, T: int, link_ee: str):
    """_retime_handle with link_ee as the end effector: the frame the payload rides on."""
    from . import _capi
    o = _capi.default_opts()
    o.T = int(T)
    o.standoff_offset = max(int(o.standoff_offset), 2 - int(T))
    return robot.solver_handle(link_ee, robot.desc.link_names[-1], o, role="util")


def retime_plans(robot, plans, vlim=None, alim=0.5, subdiv: int = 2, n_samples: int = 100, profile: str = "greedy",
                 gap_tol: float = 1e-8, max_newton=None, tau_max=None, payload=None, link_ee=None):
    """Time-optimal retiming of plans (B, ndof, T) or one plan (ndof, T) on the GPU (gto_retime_batch, include/gto_solver.h):
    not-a-knot cubic spline through the waypoints on linspace(0, 1, T), joint velocity limits ``vlim`` (default: the URDF's,
    ``robot.velocity_actuated_joint_limits``) and acceleration limits ``alim`` (default 0.5 rad/s^2, gto/utils.py:295),
    TOPP-RA's discretisation on subdiv (T-1) + 1 gridpoints, constant acceleration between them.  Returns a dict of
    duration (B,), t_grid (B, N), sd_grid (B, N), q / qd / qdd (B, n_samples, ndof) at linspace(0, duration, n_samples)
    and status (B,).  profile "greedy" (the default) is TOPP-RA's forward pass; "convex" is the time optimum of the same
    grid constraints, solved per plan to the certified relative gap ``gap_tol`` in at most ``max_newton`` Newton steps
    (gto_retime_paths_convex with Tp = T), and adds iters (B,) to the dict.  profile "torque" is that optimum under joint
    torque limits as well (gto_retime_paths_torque): ``tau_max`` ((ndof,) or one value, +inf = none; default: the URDF's
    effort limits, ``robot.desc.effort``) bounds the inverse dynamics along the path, with ``payload`` (the dict of
    ``inverse_dynamics``, one value per call or per plan) on ``link_ee``; it needs link inertials on the description and adds
    iters and tau (B, n_samples, ndof); status 3: some joint cannot hold the path at rest."""
    from . import _capi
    profile, gap_tol, max_newton = _capi.retime_profile(profile, gap_tol, max_newton)
    plans = np.asarray(plans, dtype=np.float64)
    if plans.ndim == 2:
        plans = plans[None]
    if profile == "torque":  # checked before the robot is asked for anything but its description
        tm, payload, ee = _torque_request(robot, tau_max, payload, plans.shape[0], link_ee)
    if vlim is None:
        vlim = np.asarray(robot.velocity_actuated_joint_limits.toarray()).ravel()
    if profile == "torque":
        return _torque_handle(robot, plans.shape[2], ee).retime_paths_torque(
            plans, vlim, alim, tau_max=tm, payload=payload, subdiv=subdiv, n_samples=n_samples, gap_tol=gap_tol, max_newton=max_newton)
    h = _retime_handle(robot, plans.shape[2])
    if profile == "convex":
        return h.retime_paths_convex(plans, vlim, alim, subdiv=subdiv, n_samples=n_samples, gap_tol=gap_tol, max_newton=max_newton)
    return h.retime_batch(plans, vlim, alim, subdiv=subdiv, n_samples=n_samples)


def retime_paths(robot, paths, n_cols=None, vlim=None, alim=0.5, subdiv: int = 2, n_samples: int = 100,
                 profile: str = "greedy", gap_tol: float = 1e-8, max_newton=None, tau_max=None, payload=None, link_ee=None):
    """``retime_plans`` for paths (B, ndof, Tp) or one path (ndof, Tp) of any length Tp >= 2 (gto_retime_paths,
    include/gto_solver.h): a retrieve path of ``GTOPlanner.retrieve_path``, for one.  n_cols (B,) int or None: path b is its
    first n_cols[b] columns and the rest is ignored (a lift up to the step it reached: ``reached + 1``); t_grid and sd_grid
    are (B, subdiv (Tp-1) + 1) and hold the duration and 0 past a path's own gridpoints.  One handle serves every Tp.
    profile, gap_tol, max_newton, tau_max, payload, link_ee: as in ``retime_plans`` (gto_retime_paths_convex,
    gto_retime_paths_torque)."""
    from . import _capi
    profile, gap_tol, max_newton = _capi.retime_profile(profile, gap_tol, max_newton)
    paths = np.asarray(paths, dtype=np.float64)
    if paths.ndim == 2:
        paths = paths[None]
    if profile == "torque":
        tm, payload, ee = _torque_request(robot, tau_max, payload, paths.shape[0], link_ee)
    if vlim is None:
        vlim = np.asarray(robot.velocity_actuated_joint_limits.toarray()).ravel()
    if profile == "torque":
        return _torque_handle(robot, 4, ee).retime_paths_torque(
            paths, vlim, alim, tau_max=tm, payload=payload, n_cols=n_cols, subdiv=subdiv, n_samples=n_samples, gap_tol=gap_tol,
            max_newton=max_newton)
    h = _retime_handle(robot, 4)
    if profile == "convex":
        return h.retime_paths_convex(paths, vlim, alim, n_cols=n_cols, subdiv=subdiv, n_samples=n_samples, gap_tol=gap_tol,
                                     max_newton=max_newton)
    return h.retime_paths(paths, vlim, alim, n_cols=n_cols, subdiv=subdiv, n_samples=n_samples)


def self_clearance(robot, plans, clearance=None, cutoff=None, mask=None, q_ref=None):
    """The robot's distance from itself along ``plans`` (B, ndof, Tp) or (ndof, Tp), any Tp >= 1, on the GPU
    (gto_self_clearance): what the reference learns when PyBullet executes a plan that folds the arm into itself
    (examples/pybullet_gto_planning.py:301).  clearance: metres, default the description's point_spacing(); cutoff: default
    2 x clearance (distances beyond it are reported as the cutoff, with pair (-1, -1)); mask: (L, L) bool link pairs,
    default ``RobotDesc.self_pairs(q_ref, clearance)``; q_ref: a pose known to be good, e.g. the config's default_pose.
    Returns a dict: d2 (squared metres), dist, pair (.., 2), clear = dist >= clearance (a column with a non-finite entry
    has d2 = NaN and is not clear)."""
    from ._capi import self_check_request
    plans = np.asarray(plans, dtype=np.float64)
    single = plans.ndim == 2
    paths = np.ascontiguousarray(plans.reshape(-1, robot.desc.ndof, plans.shape[-1]))
    clearance, cutoff, mask = self_check_request(robot.desc, dict(clearance=clearance, cutoff=cutoff, mask=mask, q_ref=q_ref))
    h = _retime_handle(robot, 50)
    h.set_self_pairs(mask)
    out = h.self_clearance(paths, cutoff=cutoff)
    with np.errstate(invalid="ignore"):
        out["clear"] = out["dist"] >= clearance
    return {k: v[0] for k, v in out.items()} if single else out


def held_clearance(robot, paths, link_ee, held_points, n_held=None, attach=None, attach_col=None, object_pose=None,
                   base_position=(0.0, 0.0, 0.0), clearance=None, cutoff=None, links=None, ignore=()):
    """The held object's distance from the robot's own links along ``paths`` (B, ndof, Tp) or (ndof, Tp), any Tp >= 1, on
    the GPU (gto_held_clearance): the object rides with ``link_ee`` from the grasp configuration -- column 0 of the path,
    or column ``attach_col`` (default: the last) of ``attach`` -- and a wrist that folds back drives it into the forearm or
    the base, which no other check sees.  held_points / n_held / object_pose: as ``SolverHandle.check_held_paths`` takes
    them (one (n, 3) array for one path).  clearance: metres, default the description's point_spacing(); cutoff: default
    2 x clearance (distances beyond it are reported as the cutoff, with link and point -1); links: (L,) bool, default
    ``RobotDesc.held_links(link_ee, ignore)``.  Returns a dict: d2 (squared metres), dist, link, point, clear = dist >=
    clearance (a column with a non-finite entry has d2 = NaN and is not clear)."""
    from ._capi import held_clearance_request
    paths = np.asarray(paths, dtype=np.float64)
    single = paths.ndim == 2
    paths = np.ascontiguousarray(paths.reshape(-1, robot.desc.ndof, paths.shape[-1]))
    clearance, cutoff, links = held_clearance_request(robot.desc, link_ee, dict(clearance=clearance, cutoff=cutoff, links=links,
                                                                                ignore=ignore))
    if single:
        if n_held is None and isinstance(held_points, np.ndarray) and held_points.ndim == 2:
            held_points = [held_points]
        attach = None if attach is None else np.asarray(attach, dtype=np.float64).reshape(1, robot.desc.ndof, -1)
    out = _torque_handle(robot, 50, link_ee).held_clearance(paths, held_points, n_held=n_held, attach=attach, attach_col=attach_col,
                                                            object_pose=object_pose, base_pos=base_position, links=links,
                                                            cutoff=cutoff)
    with np.errstate(invalid="ignore"):
        out["clear"] = out["dist"] >= clearance
    return {k: v[0] for k, v in out.items()} if single else out


def inverse_dynamics(robot, q, qd, qdd, payload=None, link_ee=None):
    """Joint forces tau = M(q) qdd + C(q, qd) qd + g(q) of states (n, ndof) or one state (ndof,) on the GPU
    (gto_inverse_dynamics, include/gto_solver.h): recursive Newton-Euler over the robot's frames with the link inertials of
    ``robot.desc`` (a description built from a URDF has them; one loaded from the packaged files gets them with
    ``robot.desc.set_link_inertials``).  payload: None, or a dict with "mass" and optionally "com" and "inertia" (ixx ixy ixz
    iyy iyz izz about that centre), each one value or one per state: a rigid body on ``link_ee``, stated in that link's
    frame.  Returns (n, ndof), N m (N for a prismatic joint)."""
    q = np.asarray(q, dtype=np.float64)
    one = q.ndim == 1
    if not robot.desc.has_inertials:
        raise ValueError("inverse_dynamics: the robot description has no link inertials (RobotDesc.set_link_inertials)")
    if payload is not None and link_ee is None:
        raise ValueError("inverse_dynamics: a payload needs link_ee, the link that carries it")
    ln = robot.desc.link_names[-1] if link_ee is None else link_ee
    tau = robot.solver_handle(ln, robot.desc.link_names[-1], role="util").inverse_dynamics(q, qd, qdd, payload)
    return tau[0] if one else tau


def forward_dynamics(robot, q, qd, tau, payload=None, link_ee=None, locked=None):
    """Joint accelerations that the forces ``tau`` cause at states (n, ndof) or one state (ndof,) on the GPU
    (gto_forward_dynamics, include/gto_solver.h): the inverse of ``inverse_dynamics`` on the free joints, with the same
    inertials and payload rules.  locked: None (every joint that is not optimised stands still: Panda's fingers, Fetch's
    torso and head) or one flag per joint; locked joints get 0.  Returns (n, ndof); a row with a non-finite entry, or with a
    free joint that moves no mass, is NaN."""
    q = np.asarray(q, dtype=np.float64)
    one = q.ndim == 1
    if not robot.desc.has_inertials:
        raise ValueError("forward_dynamics: the robot description has no link inertials (RobotDesc.set_link_inertials)")
    if payload is not None and link_ee is None:
        raise ValueError("forward_dynamics: a payload needs link_ee, the link that carries it")
    ln = robot.desc.link_names[-1] if link_ee is None else link_ee
    qdd = robot.solver_handle(ln, robot.desc.link_names[-1], role="util").forward_dynamics(q, qd, tau, payload, locked)[0]
    return qdd[0] if one else qdd


def track_trajectories(robot, retimed, kp, kd, tau_max=None, dt=1e-3, settle=0.0, n_samples=100, feedforward="full",
                       model_payload=None, plant_payload=None, locked=None, link_ee=None):
    """Roll retimed trajectories forward under a torque-limited joint controller on the GPU (gto_track_rollout,
    include/gto_solver.h).  retimed: the dict any ``retime_plans`` / ``retime_paths`` profile returns (duration (B,), q / qd /
    qdd (B, M, ndof)).  Every ``dt`` the controller sets tau = clip(ff + kp (q_ref - q) + kd (qd_ref - qd), +-tau_max) and
    holds it while the plant integrates (RK4); ``settle`` seconds follow the reference's end.  kp, kd: one value or one per
    joint; tau_max: None = the description's effort limits; feedforward: "none", "gravity" (the model's holding torque at
    q_ref) or "full" (its inverse dynamics along the reference).  model_payload is what the controller believes the hand
    holds, plant_payload what it holds (each the dict of ``inverse_dynamics`` on ``link_ee``, one value or one per
    trajectory).  locked: as in ``forward_dynamics``; locked joints stand at the reference's start.  Returns a dict: q, qd
    (B, n_samples, ndof) and t (B, n_samples), the state after step floor(m steps / (n_samples - 1)); err_max, err_end
    (B,), the largest and the last |q - q_ref| over the free joints; sat_steps, steps, status (B,) (2: NaN outputs)."""
    from . import _capi
    if not robot.desc.has_inertials:
        raise ValueError("track_trajectories: the robot description has no link inertials (RobotDesc.set_link_inertials)")
    missing = [k for k in ("duration", "q", "qd", "qdd") if k not in retimed]
    if missing:
        raise ValueError(f"track_trajectories: retimed lacks {missing}: the dict of retime_plans / retime_paths expected")
    B = np.shape(retimed["duration"])[0]
    _capi.track_controller(robot.desc, kp, kd, tau_max, dt, settle, n_samples, feedforward, locked)
    for pl in (model_payload, plant_payload):
        _capi.payload_arrays(pl, B)
        if pl is not None and link_ee is None:
            raise ValueError("track_trajectories: a payload needs link_ee, the link that carries it")
    ln = robot.desc.link_names[-1] if link_ee is None else link_ee
    h = robot.solver_handle(ln, robot.desc.link_names[-1], role="util")
    return h.track_rollout(retimed["duration"], retimed["q"], retimed["qd"], retimed["qdd"], kp, kd, tau_max=tau_max, dt=dt,
                           settle=settle, n_samples=n_samples, feedforward=feedforward, model_payload=model_payload,
                           plant_payload=plant_payload, locked=locked)


def convert_plan_to_trajectory_toppra(robot, plan, is_show: bool = False):
    """gto/utils.py:283-323 on the GPU: plan (ndof, T) -> (qs_sample, qds_sample, qdds_sample, ts_sample), 100 samples of
    each, in the reference's order.  Velocity limits from the URDF for all ndof joints (the reference passes the n_opt
    optimised ones for an ndof path; parameter rows of a solved plan are constant, so their limits have no effect),
    acceleration limits 0.5.  The gridpoints are fixed (retime_plans, subdiv=2) where toppra picks them adaptively."""
    if is_show:
        raise NotImplementedError("convert_plan_to_trajectory_toppra(is_show=True): plotting is not ported")
    r = retime_plans(robot, np.asarray(plan, dtype=np.float64)[None], n_samples=100)
    ts = np.linspace(0.0, r["duration"][0], 100)
    return r["q"][0], r["qd"][0], r["qdd"][0], ts
