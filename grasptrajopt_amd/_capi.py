"""ctypes binding of the C ABI in include/gto_solver.h (libgto_hip.so).

There is deliberately NO fallback: if the HIP library is missing or no GPU is present the calls
raise.  (The CPU oracle under oracle/ is test infrastructure and is never imported from here.)
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .robot_desc import RobotDesc

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GTO_HIP_LIB", os.path.join(_HERE, "csrc", "libgto_hip.so"))  # override: A/B builds

# include/gto_solver.h
GTO_MAX_FRAMES, GTO_MAX_LINKS, GTO_MAX_OPT, GTO_MAX_DOF = 32, 32, 16, 32
GTO_GRAD_CENTRAL_DIFF, GTO_GRAD_ZERO = 0, 1
GTO_STATUS_CONVERGED, GTO_STATUS_MAX_ITER, GTO_STATUS_NUMERICAL = 0, 1, 2
ABI_VERSION = 1012  # GTO_ABI_VERSION (checked against gto_version() when the library is loaded)

_pd = C.POINTER(C.c_double)
_pi = C.POINTER(C.c_int32)
_pf = C.POINTER(C.c_float)


class CRobotDesc(C.Structure):
    _fields_ = [
        ("n_frames", C.c_int32), ("parent", _pi), ("joint_type", _pi), ("q_index", _pi),
        ("origin_xyz", _pd), ("origin_rpy", _pd), ("axis", _pd),
        ("ndof", C.c_int32), ("n_opt", C.c_int32), ("opt_index", _pi), ("lower", _pd), ("upper", _pd),
        ("n_links", C.c_int32), ("link_frame", _pi), ("visual_xyz", _pd), ("visual_rpy", _pd),
        ("n_points", C.c_int32), ("points", _pd), ("point_link", _pi),
        ("frame_ee", C.c_int32), ("frame_gripper", C.c_int32),
        ("n_gripper_points", C.c_int32), ("gripper_points", _pd),
    ]


class CSolverOpts(C.Structure):
    _fields_ = [
        ("T", C.c_int32), ("Tmax", C.c_double), ("standoff_offset", C.c_int32),
        ("w_obstacle", C.c_double), ("w_vel", C.c_double), ("max_iter", C.c_int32),
        ("tol_step", C.c_double), ("tol_rel_f", C.c_double), ("lambda0", C.c_double),
        ("grad_mode", C.c_int32),
    ]

    def copy(self) -> "CSolverOpts":
        o = CSolverOpts()
        C.memmove(C.byref(o), C.byref(self), C.sizeof(CSolverOpts))
        return o


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a: Optional[np.ndarray], typ):
    return None if a is None else a.ctypes.data_as(typ)


def _vp(a):
    """A device pointer or a stream (an int such as torch.Tensor.data_ptr()) or None."""
    return None if a is None else C.c_void_p(int(a))


def _per_instance(x, B) -> np.ndarray:
    """One int32 per instance from a scalar or an array (B,)."""
    return _i32(np.broadcast_to(np.asarray(x), (B,)))


def _bases(base_pos, B) -> np.ndarray:
    """One base position per instance, (B, 3), from (3,) or (B, 3)."""
    return _f64(np.broadcast_to(_f64(base_pos).reshape(-1, 3), (B, 3)))


def _prototypes():
    """Every entry point of include/gto_solver.h, in its order: name -> (restype, argtypes).  The only place where this
    binding states a signature; tests/test_capi_cpu.py compares it with the header argument by argument."""
    I, I32, I64, D, F = C.c_int, C.c_int32, C.c_int64, C.c_double, C.c_float
    V = C.c_void_p  # gto_handle*, gto_observation*, gto_occupancy*, device pointers and streams
    PV = C.POINTER(V)  # out-handles, void* const*
    pu8, pu64 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    desc, opts = C.POINTER(CRobotDesc), C.POINTER(CSolverOpts)
    solve = [V, I32, I32] + [V] * 12
    scene = [V, I32, _pf, _pf, _pi, _pd, D]
    depth = [I, _pf, I32, I32, _pd, _pd, _pd, _pd, pu8, D]  # device, image, camera, mask, threshold
    seeds = [V] * 7 + [I32, I32]
    return {
        "gto_default_opts": (None, [opts]),
        "gto_version": (I32, []),
        "gto_create": (I, [desc, opts, I, PV]),
        "gto_destroy": (None, [V]),
        "gto_last_error": (C.c_char_p, [V]),
        "gto_set_opts": (I, [V, opts]),
        "gto_set_scene": (I, scene),
        "gto_set_scene_values": (I, scene),
        "gto_drop_scene": (I, [V, I32]),
        "gto_solve_batch": (I, solve),
        "gto_solve_batch_device": (I, solve + [V]),
        "gto_share_scene": (I, [V, I32, V, I32]),
        "gto_share_scene_halves": (I, [V, I32, V, I32, I32, I32]),
        "gto_solve_ik_batch": (I, [V, I32, _pi, _pd, _pd, _pd, I32, _pd, _pd, _pi, _pi]),
        "gto_solve_ik_pose_batch": (I, [V, I32, I32, _pi, _pd, _pd, _pd, I32, _pd, _pd, _pi, _pi]),
        "gto_solve_base_batch": (I, [V, I32, I32, _pi, _pd, _pd, D, I32, _pd, _pd, _pd, _pi, _pi]),
        "gto_set_mode": (I, [V, I32]),
        "gto_set_lanes": (I, [V, I32, I32, I32]),
        "gto_set_lane_streams": (I, [V, I32, PV]),
        "gto_set_stream": (I, [V, V]),
        "gto_last_kernel_time": (I, [V, _pd, _pi]),
        "gto_last_kernel_work": (I, [V, pu64, pu64]),
        "gto_last_kernel_profile": (I, [V, I32, _pd, _pi, pu64, pu64]),
        "gto_set_profiling": (I, [V, I32]),
        "gto_eval_fk": (I, [V, I32, _pd, _pd]),
        "gto_eval_points": (I, [V, I32, I32, _pd, _pd, I32, _pd, _pi, _pd, _pd]),
        "gto_eval_points_hessian": (I, [V, I32, I32, _pd, _pd, I32, _pd]),
        "gto_set_link_inertials": (I, [V, _pd, _pd, _pd, _pd]),
        "gto_inverse_dynamics": (I, [V, I32, _pd, _pd, _pd, _pd, _pd, _pd, _pd]),
        "gto_eval_objective": (I, [V, I32, I32, _pi, _pd, _pi, _pd, _pd, _pd, _pd, _pd, _pd, _pi]),
        "gto_eval_obstacle_normal_eq": (I, [V, I32, _pi, _pd, _pd, _pd, _pd, _pd]),
        "gto_eval_base_objective": (I, [V, I32, I32, _pi, _pd, _pd, _pd, D, _pd]),
        "gto_plan_cost": (I, [V, I32, I32, _pd, _pd, _pd, _pd]),
        "gto_depth_sdf_cost": (I, depth + [_pd, I64, F, F, _pf, pu8, _pf, _pd, pu8]),
        "gto_scene_from_depth": (I, [V, I32, _pf, I32, I32, _pd, _pd, _pd, _pd, pu8, _pf, D, D, D, F, F, _pi, _pd, _pd]),
        "gto_cloud_sdf_cost": (I, [I, _pd, _pd, I64, I32, _pd, I64, F, F, _pf, pu8, _pf, _pi]),
        "gto_scene_from_clouds": (I, [V, I32, _pd, _pd, I64, I64, I32, D, D, F, F, _pi, _pd, _pd]),
        "gto_get_scene_fields": (I, [V, I32, _pf, _pf]),
        "gto_observation_from_depth": (I, depth + [PV]),
        "gto_observation_from_cloud": (I, [I, _pd, _pd, I64, I32, PV]),
        "gto_observation_destroy": (None, [V]),
        "gto_observation_sdf": (I, [V, _pd, I64, _pf, pu8]),
        "gto_observation_check_posed": (I, [V, _pd, I32, _pd, I32, _pi]),
        "gto_check_plans": (I, [V, V, I32, _pd, _pd, I32, _pi]),
        "gto_check_plans_device": (I, [V, V, I32, V, _pd, I32, V, V]),
        "gto_retime_batch": (I, [V, I32, _pd, _pd, _pd, I32, I32, _pd, _pd, _pd, _pd, _pd, _pd, _pi]),
        "gto_retime_batch_device": (I, [V, I32, V, _pd, _pd, I32, I32] + [V] * 8),
        "gto_solve_ik_pose_batch_device": (I, [V, I32, I32] + [V] * 4 + [I32] + [V] * 5),
        "gto_ik_report_device": (I, [V, I32] + [V] * 4 + [D] * 3 + [V] * 5),
        "gto_seed_goalsets_device": (I, [V, I32, I32] + seeds + [V] * 8),
        "gto_occupancy_from_observation": (I, [V, D, D, D, PV]),
        "gto_occupancy_from_points": (I, [I, _pd, I64, D, D, D, PV]),
        "gto_occupancy_geometry": (I, [V, _pd, _pi, _pd, _pd]),
        "gto_occupancy_grid": (I, [V, pu8]),
        "gto_occupancy_destroy": (None, [V]),
        "gto_solve_base_batch_device": (I, [V, I32, I32, _pi, V, V, D, I32] + [V] * 6),
        "gto_base_report_device": (I, [V, V, I32, I32, _pi] + [V] * 9),
        "gto_seed_goalsets_multi_device": (I, [V, I32, I32, I32] + seeds + [V] * 9),
        "gto_plan_report_device": (I, [V, I32, I32] + [V] * 9),
        "gto_select_plans_device": (I, [V, I32, I32] + [V] * 5 + [D, D, I32] + [V] * 7),
        "gto_filter_grasps_device": (I, [V, I32, I32, PV, V, I32] + [V] * 5 + [_pd, _pd, D] + [V] * 8),
        "gto_retrieve_lift_device": (I, [V, I32, V, V, V, _pd, D, I32, _pi, _pd, I32, I32, D, D] + [V] * 8),
        "gto_retrieve_lift": (I, [V, I32, _pd, _pi, _pd, _pd, D, I32, _pi, _pd, I32, I32, D, D, _pd, _pd, _pd, _pd, _pi, _pi, _pi]),
        "gto_retrieve_reverse_device": (I, [V, I32, V, _pi, _pd, I32, V, _pi, V]),
        "gto_retrieve_path_columns": (I, [V]),
        "gto_check_paths": (I, [V, V, I32, I32, _pd, _pd, I32, _pi]),
        "gto_check_paths_device": (I, [V, V, I32, I32, V, _pd, I32, V, V]),
        "gto_check_held_paths": (I, [V, V, I32, I32, _pd, _pd, I32, I32, _pd, I32, _pi, _pd, _pi, _pi, _pd, I32, _pi]),
        "gto_check_held_paths_device": (I, [V, V, I32, I32, V, V, I32, I32, V, I32, V, V, V, V, _pd, I32, V, V]),
        "gto_retime_paths": (I, [V, I32, I32, _pd, _pi, _pd, _pd, I32, I32, _pd, _pd, _pd, _pd, _pd, _pd, _pi]),
        "gto_retime_paths_device": (I, [V, I32, I32, V, V, _pd, _pd, I32, I32] + [V] * 8),
        "gto_retime_paths_convex": (I, [V, I32, I32, _pd, _pi, _pd, _pd, I32, I32, D, I32, _pd, _pd, _pd, _pd, _pd, _pd, _pi, _pi]),
        "gto_retime_paths_convex_device": (I, [V, I32, I32, V, V, _pd, _pd, I32, I32, D, I32] + [V] * 9),
        "gto_retime_paths_torque": (I, [V, I32, I32, _pd, _pi, _pd, _pd, _pd, _pd, _pd, _pd, I32, I32, D, I32, _pd, _pd, _pd, _pd,
                                        _pd, _pd, _pd, _pi, _pi]),
        "gto_retime_paths_torque_device": (I, [V, I32, I32, V, V, _pd, _pd, _pd, V, V, V, I32, I32, D, I32] + [V] * 10),
        "gto_forward_dynamics": (I, [V, I32, _pd, _pd, _pd, _pd, _pd, _pd, _pi, _pd, _pd, _pi]),
        "gto_track_rollout": (I, [V, I32, I32] + [_pd] * 7 + [D, D, I32] + [_pd] * 6 + [_pi, I32] + [_pd] * 5 + [_pi] * 3),
        "gto_track_rollout_device": (I, [V, I32, I32] + [V] * 4 + [_pd] * 3 + [D, D, I32] + [V] * 6 + [_pi, I32] + [V] * 9),
        "gto_set_self_pairs": (I, [V, _pi]),
        "gto_self_clearance": (I, [V, I32, I32, _pd, D, _pd, _pi]),
        "gto_self_clearance_device": (I, [V, I32, I32, V, D, V, V, V]),
        "gto_held_clearance": (I, [V, I32, I32, _pd, _pd, I32, I32, _pd, I32, _pi, _pd, _pd, I32, I32, D, _pd, _pi, _pi]),
        "gto_held_clearance_device": (I, [V, I32, I32, V, V, I32, I32, V, I32, V, V, _pd, I32, I32, D, V, V, V, V]),
    }


PROTOTYPES = _prototypes()
# Newton steps a path may take in the convex retiming by default: more than twice the largest count seen over the test
# inputs
RETIME_MAX_NEWTON = 400
RETIME_PROFILES = ("greedy", "convex", "torque")
STATUS_INFEASIBLE = 3  # GTO_STATUS_INFEASIBLE: a joint cannot hold the path at rest under its torque limit
TRACK_FEEDFORWARD = {"none": 0, "gravity": 1, "full": 2}  # the feedforward of gto_track_rollout by name
TRACK_KEYS = ("q", "qd", "t", "err_max", "err_end", "sat_steps", "steps", "status")


def retime_profile(profile="greedy", gap_tol=1e-8, max_newton=None):
    """The checked (profile, gap_tol, max_newton) of a retime request, for every Python layer that takes one."""
    if profile not in RETIME_PROFILES:
        raise ValueError(f"retime: profile must be one of {RETIME_PROFILES}, got {profile!r}")
    gap_tol = float(gap_tol)
    if not (np.isfinite(gap_tol) and gap_tol > 0):
        raise ValueError(f"retime: gap_tol must be finite and > 0, got {gap_tol}")
    max_newton = RETIME_MAX_NEWTON if max_newton is None else int(max_newton)
    if max_newton < 1:
        raise ValueError(f"retime: max_newton must be >= 1, got {max_newton}")
    return profile, gap_tol, max_newton
EXPORTED_SYMBOLS = tuple(PROTOTYPES)


def self_pair_rows(mask, n_links):
    """The words gto_set_self_pairs takes, int32 (L,), of an (L, L) link-pair mask: bit b of word a is mask[a, b].  The
    library judges symmetry and the diagonal."""
    m = np.asarray(mask)
    if m.shape != (n_links, n_links):
        raise ValueError(f"set_self_pairs: the mask must be ({n_links}, {n_links}), got shape {m.shape}")
    words = ((m != 0).astype(np.uint64) << np.arange(n_links, dtype=np.uint64)[None, :]).sum(axis=1)
    return words.astype(np.uint32).view(np.int32)


SELF_CHECK_OPTIONS = frozenset(("clearance", "cutoff", "mask", "q_ref"))  # the keys of a self_check= request


def self_check_request(desc, spec):
    """The checked (clearance, cutoff, mask) of a self-clearance request, for every Python layer that takes one.  ``spec``:
    a dict with any of ``clearance`` (metres, > 0; default: the description's point_spacing(), a property of the sampling),
    ``cutoff`` (metres, > 0, +inf allowed; default 2 x clearance: beyond it the check reports "far" and costs little),
    ``mask`` ((L, L) bool; default RobotDesc.self_pairs at ``q_ref`` with this clearance) and ``q_ref`` (ndof,): a pose known
    to be good, the configs' default_pose, whose close pairs say nothing."""
    spec = {} if spec is None else dict(spec)
    if set(spec) - SELF_CHECK_OPTIONS:
        raise TypeError(f"self_check: unexpected key(s) {sorted(set(spec) - SELF_CHECK_OPTIONS)}")
    clearance = desc.point_spacing() if spec.get("clearance") is None else float(spec["clearance"])
    cutoff = 2.0 * clearance if spec.get("cutoff") is None else float(spec["cutoff"])
    if not clearance > 0 or not cutoff > 0:
        raise ValueError(f"self_check: clearance and cutoff must be > 0, got {clearance} and {cutoff}")
    mask = spec.get("mask")
    if mask is None:
        mask = desc.self_pairs(q_ref=spec.get("q_ref"), clearance=clearance)
    self_pair_rows(mask, desc.n_links)  # (the shape)
    return clearance, cutoff, np.asarray(mask) != 0


def self_check_summary(d2, pair, clearance, prefix="self_"):
    """Per path, from the per-column d2 (B, Tp) and pair (B, Tp, 2) of gto_self_clearance: <prefix>d2 (B,) the smallest d2
    over the columns (NaN if a column is NaN), <prefix>pair (B, 2) the pair at that column ((-1, -1) for NaN or far) and
    <prefix>clear (B,) bool: every column's distance is at least ``clearance`` (a NaN column is not clear)."""
    d2, pair = np.asarray(d2), np.asarray(pair)
    B = d2.shape[0]
    bad = np.isnan(d2).any(axis=1)
    col = np.where(bad, np.isnan(d2).argmax(axis=1), np.where(np.isnan(d2), np.inf, d2).argmin(axis=1))
    rows = np.arange(B)
    return {prefix + "d2": d2[rows, col], prefix + "pair": pair[rows, col].astype(np.int32),
            prefix + "clear": ~bad & (np.sqrt(np.where(np.isnan(d2), 0.0, d2)) >= clearance).all(axis=1)}


def held_link_mask(links, n_links):
    """The link_mask word of gto_held_clearance (a Python int, the bits of an unsigned 32-bit word as int32) of an (L,)
    bool array of enabled collision links."""
    m = np.asarray(links)
    if m.shape != (n_links,):
        raise ValueError(f"held_clearance: links must be ({n_links},), got shape {m.shape}")
    word = sum(1 << l for l in range(n_links) if m[l])
    return int(np.array([word], dtype=np.uint32).view(np.int32)[0])


HELD_CLEARANCE_OPTIONS = frozenset(("clearance", "cutoff", "links", "ignore"))  # the keys of a held_clearance= request


def held_clearance_request(desc, link_ee, spec):
    """The checked (clearance, cutoff, links) of a held-clearance request, for every Python layer that takes one.  ``spec``:
    a dict with any of ``clearance`` (metres, > 0; default: the description's point_spacing()), ``cutoff`` (metres, > 0,
    +inf allowed; default 2 x clearance: beyond it the check reports "far" and costs little), ``links`` ((L,) bool, the
    collision links the held object is measured against; default RobotDesc.held_links(link_ee, ignore)) and ``ignore``
    (link names the default leaves out)."""
    spec = {} if spec is None else dict(spec)
    if set(spec) - HELD_CLEARANCE_OPTIONS:
        raise TypeError(f"held_clearance: unexpected key(s) {sorted(set(spec) - HELD_CLEARANCE_OPTIONS)}")
    clearance = desc.point_spacing() if spec.get("clearance") is None else float(spec["clearance"])
    cutoff = 2.0 * clearance if spec.get("cutoff") is None else float(spec["cutoff"])
    if not clearance > 0 or not cutoff > 0:
        raise ValueError(f"held_clearance: clearance and cutoff must be > 0, got {clearance} and {cutoff}")
    links = spec.get("links")
    if links is None:
        links = desc.held_links(link_ee, ignore=spec.get("ignore") or ())
    elif spec.get("ignore"):
        links = np.array(links, dtype=bool)
        links[[desc.link_names.index(n) for n in spec["ignore"]]] = False
    held_link_mask(links, desc.n_links)  # (the shape)
    return clearance, cutoff, np.asarray(links) != 0


def held_clearance_summary(d2, link, point, clearance, prefix="held_self_"):
    """Per path, from the per-column d2, link and point (B, Tp) of gto_held_clearance: <prefix>d2 (B,) the smallest d2 over
    the columns (NaN if a column is NaN), <prefix>col (B,) that column (the first NaN column of a path with one),
    <prefix>link and <prefix>point (B,) the link and the held point there (-1 for NaN or far) and <prefix>clear (B,) bool:
    every column's distance is at least ``clearance`` (a NaN column is not clear)."""
    d2, link, point = np.asarray(d2), np.asarray(link), np.asarray(point)
    B = d2.shape[0]
    bad = np.isnan(d2).any(axis=1)
    col = np.where(bad, np.isnan(d2).argmax(axis=1), np.where(np.isnan(d2), np.inf, d2).argmin(axis=1))
    rows = np.arange(B)
    return {prefix + "d2": d2[rows, col], prefix + "col": col.astype(np.int32), prefix + "link": link[rows, col].astype(np.int32),
            prefix + "point": point[rows, col].astype(np.int32),
            prefix + "clear": ~bad & (np.sqrt(np.where(np.isnan(d2), 0.0, d2)) >= clearance).all(axis=1)}


def retime_torque_limits(desc, tau_max=None, need_inertials=True):
    """The checked joint torque limits (ndof,) of a profile="torque" request: ``tau_max`` (one value or one per joint, > 0,
    +inf = no limit), None = the description's effort limits.  Raises ValueError for anything else and for a description
    without link inertials, which the torque rows need (need_inertials=False leaves that to the library)."""
    if need_inertials and not desc.has_inertials:
        raise ValueError("retime: profile 'torque' needs link inertials on the robot description (RobotDesc.set_link_inertials)")
    if tau_max is None:
        if desc.effort is None:
            raise ValueError("retime: tau_max=None takes the description's effort limits, and it records none")
        tau_max = desc.effort
    try:
        tm = _f64(np.broadcast_to(np.asarray(tau_max, dtype=np.float64), (desc.ndof,)))
    except ValueError:
        raise ValueError(f"retime: tau_max must be one value or ({desc.ndof},), got shape {np.shape(tau_max)}") from None
    if not np.all(tm > 0):  # a NaN among them
        raise ValueError("retime: tau_max must be > 0 (+inf: no limit)")
    return tm


def track_controller(desc, kp, kd, tau_max=None, dt=1e-3, settle=0.0, n_samples=100, feedforward="full", locked=None,
                     need_inertials=True):
    """The checked host arguments of a rollout request, for every Python layer that takes one: (kp, kd, tau_max (ndof,),
    dt, settle, n_samples, feedforward 0 / 1 / 2, locked (ndof,) int32 or None).  Gains: one value or one per joint, finite
    and >= 0; tau_max: retime_torque_limits' rules (None = the description's effort limits); feedforward: a name of
    TRACK_FEEDFORWARD or its number; locked: None (every joint that is not optimised) or one flag per joint.  A description
    without link inertials is refused (need_inertials=False leaves that to the library)."""
    def gains(x, what):
        try:
            a = _f64(np.broadcast_to(np.asarray(x, dtype=np.float64), (desc.ndof,)))
        except ValueError:
            raise ValueError(f"track: {what} must be one value or ({desc.ndof},), got shape {np.shape(x)}") from None
        if not (np.isfinite(a).all() and (a >= 0).all()):
            raise ValueError(f"track: {what} must be finite and >= 0")
        return a

    kp, kd = gains(kp, "kp"), gains(kd, "kd")
    tm = retime_torque_limits(desc, tau_max, need_inertials)
    dt, settle, n_samples = float(dt), float(settle), int(n_samples)
    if not (np.isfinite(dt) and dt > 0):
        raise ValueError(f"track: dt must be finite and > 0, got {dt}")
    if not (np.isfinite(settle) and settle >= 0):
        raise ValueError(f"track: settle must be finite and >= 0, got {settle}")
    if n_samples < 2:
        raise ValueError(f"track: n_samples must be >= 2, got {n_samples}")
    ff = TRACK_FEEDFORWARD.get(feedforward, feedforward)
    if isinstance(ff, bool) or ff not in (0, 1, 2):
        raise ValueError(f"track: feedforward must be one of {sorted(TRACK_FEEDFORWARD)} or 0, 1, 2, got {feedforward!r}")
    if locked is not None:
        lk = np.asarray(locked)
        if lk.shape != (desc.ndof,):
            raise ValueError(f"track: locked must be ({desc.ndof},), got shape {lk.shape}")
        locked = _i32(lk != 0)
    return kp, kd, tm, dt, settle, n_samples, int(ff), locked


def payload_arrays(payload, n):
    """(mass (n,), com (n, 3) or None, inertia (n, 6) or None) of a payload request: None, or a dict with "mass" and
    optionally "com" and "inertia", each given once for the call or once per row.  (None, None, None) without a payload."""
    if payload is None:
        return None, None, None
    unknown = set(payload) - {"mass", "com", "inertia"}
    if unknown or "mass" not in payload:
        raise ValueError(f"payload: a dict with 'mass' and optionally 'com', 'inertia' expected, got keys {sorted(payload)}")

    def rows(x, width):
        a = _f64(x)
        a = a.reshape(-1, width) if a.size != width or a.ndim > 1 else a.reshape(1, width)
        if a.shape[0] not in (1, n):
            raise ValueError(f"payload: one value or {n} rows of {width} expected, got shape {np.shape(x)}")
        return _f64(np.broadcast_to(a, (n, width)))

    mass = rows(payload["mass"], 1).reshape(n)
    if not (np.isfinite(mass).all() and (mass >= 0).all()):
        raise ValueError("payload: mass must be finite and >= 0")
    com = None if payload.get("com") is None else rows(payload["com"], 3)
    inertia = None if payload.get("inertia") is None else rows(payload["inertia"], 6)
    return mass, com, inertia


def pack_robot_desc(desc: RobotDesc, link_ee: str, link_gripper: str,
                    n_gripper_points: Optional[int] = None) -> Tuple[CRobotDesc, list]:
    """Build the C struct; the returned list keeps the backing arrays alive."""
    keep: List[np.ndarray] = []

    def k(a):
        keep.append(a)
        return a

    gp = desc.link_points(link_gripper)  # gto/gto_planner.py:37
    if n_gripper_points is not None:
        gp = gp[:n_gripper_points]
    opt = desc.opt_index
    c = CRobotDesc()
    c.n_frames = desc.n_frames
    c.parent = _p(k(_i32(desc.parent)), _pi)
    c.joint_type = _p(k(_i32(desc.joint_type)), _pi)
    c.q_index = _p(k(_i32(desc.q_index)), _pi)
    c.origin_xyz = _p(k(_f64(desc.origin_xyz)), _pd)
    c.origin_rpy = _p(k(_f64(desc.origin_rpy)), _pd)
    c.axis = _p(k(_f64(desc.axis)), _pd)
    c.ndof = desc.ndof
    c.n_opt = desc.n_opt
    c.opt_index = _p(k(_i32(opt)), _pi)
    c.lower = _p(k(_f64(desc.lower[opt])), _pd)
    c.upper = _p(k(_f64(desc.upper[opt])), _pd)
    c.n_links = desc.n_links
    c.link_frame = _p(k(_i32(desc.link_frame)), _pi)
    c.visual_xyz = _p(k(_f64(desc.visual_xyz)), _pd)
    c.visual_rpy = _p(k(_f64(desc.visual_rpy)), _pd)
    c.n_points = desc.n_points
    c.points = _p(k(_f64(desc.points)), _pd)
    c.point_link = _p(k(_i32(desc.point_link)), _pi)
    c.frame_ee = desc.frame_index(link_ee)
    c.frame_gripper = desc.frame_index(link_gripper)
    c.n_gripper_points = int(gp.shape[0])
    c.gripper_points = _p(k(_f64(gp)), _pd)
    return c, keep


_lib = None


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so with the SONAME of the system
    copy (libamdhip64.so.7) but link it by file name: if libgto_hip.so pulls in /opt/rocm's copy first and torch is
    imported afterwards, a second runtime is mapped next to it and finds no devices ("No HIP GPUs are available").
    Mapping torch's copy first (when a torch is installed) makes every later lookup, by SONAME or by file, land on it.
    Only done if the bundled copy has the SONAME of the runtime the library was linked against (same ABI; otherwise a
    warning and the system runtime); GTO_PRELOAD_TORCH_HIP=0 switches it off for processes that never import torch and
    want /opt/rocm's own copy."""
    import importlib.util
    if os.environ.get("GTO_PRELOAD_TORCH_HIP") == "0":
        return None
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    for loc in (spec.submodule_search_locations if spec and spec.submodule_search_locations else []):
        cand = os.path.join(loc, "lib", "libamdhip64.so")
        if os.path.exists(cand):
            if not _same_soname(cand, os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
                import warnings
                warnings.warn(f"torch bundles a HIP runtime ({cand}) with another SONAME than /opt/rocm's: not preloading it; "
                              "import torch AFTER grasptrajopt_amd may then fail to find the GPU")
                return None
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
            return cand
    return None


def _soname(path):
    """DT_SONAME of an ELF shared object (None if it cannot be read)."""
    try:
        import re
        import subprocess
        out = subprocess.run(["readelf", "-d", os.path.realpath(path)], capture_output=True, text=True, timeout=10).stdout
        m = re.search(r"SONAME\)\s+Library soname: \[([^\]]+)\]", out)
        return m.group(1) if m else None
    except Exception:
        return None


def _same_soname(a, b):
    sa, sb = _soname(a), _soname(b)
    return sa is None or sb is None or sa == sb  # unreadable: do as before


def load_library(path: Optional[str] = None):
    """Load libgto_hip.so (built by __graft_entry__.build()). Raises if it is not there."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"HIP library not found at {p}: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the GTO solve path.")
    _preload_hip_runtime()
    lib = C.CDLL(p)
    lib.gto_version.restype = PROTOTYPES["gto_version"][0]
    # one ABI number for wrapper and library: a library named by GTO_HIP_LIB for an A/B run has to be a build of THIS
    # interface -- an older one that lacks a symbol, or has it with other arguments (gto_scene_from_depth once got a pointer
    # in the middle of its signature), is refused here instead of being called with shifted arguments
    v = int(lib.gto_version())
    if v != ABI_VERSION:
        raise RuntimeError(f"{p}: ABI version {v}, this wrapper speaks {ABI_VERSION} (include/gto_solver.h GTO_ABI_VERSION): "
                           "rebuild the library from this tree (__graft_entry__.build())")
    # entry points that were added without a new ABI number (include/gto_solver.h): a build from before them is refused by name
    missing = [sym for sym in EXPORTED_SYMBOLS if not hasattr(lib, sym)]
    if missing:
        raise RuntimeError(f"{p}: ABI version {v} but no {', '.join(missing)}: an older build of this interface; "
                           "rebuild the library from this tree (__graft_entry__.build())")
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if path is None:
        _lib = lib
    return lib


def default_opts() -> CSolverOpts:
    o = CSolverOpts()
    load_library().gto_default_opts(C.byref(o))
    return o


class GTOError(RuntimeError):
    pass


class SolverHandle:
    """Owns one gto_handle (one HIP device, one stream)."""

    def __init__(self, desc: RobotDesc, link_ee: str, link_gripper: str,
                 opts: Optional[CSolverOpts] = None, device: int = -1,
                 n_gripper_points: Optional[int] = None):
        self.lib = load_library()
        self.desc = desc
        self.opts = opts.copy() if opts is not None else default_opts()
        self._cdesc, self._keep = pack_robot_desc(desc, link_ee, link_gripper, n_gripper_points)
        h = C.c_void_p()
        rc = self.lib.gto_create(C.byref(self._cdesc), C.byref(self.opts), device, C.byref(h))
        if rc != 0:
            msg = self.lib.gto_last_error(None)
            raise GTOError(f"gto_create failed ({rc}): {msg.decode() if msg else ''}")
        self._h = h
        self.scenes = {}
        self._scene_gen = {}  # scene id -> number of times it was written (set_scene, scene_from_depth, share_scene, drop_scene)
        self._inertials = None  # the description's arrays this handle uploaded last (sync_link_inertials)
        self.sync_link_inertials()

    # -------------------------------------------------------------- helpers
    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.gto_last_error(self._h)
            raise GTOError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "_h", None):
            self.lib.gto_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def T(self) -> int:
        return int(self.opts.T)

    def set_opts(self, **kw):
        new = self.opts.copy()  # a refused call leaves self.opts as the library still has them
        for k, v in kw.items():
            if not hasattr(new, k):
                raise AttributeError(k)
            setattr(new, k, v)
        self._check(self.lib.gto_set_opts(self._h, C.byref(new)), "gto_set_opts")
        self.opts = new

    def set_scene(self, scene_id: int, c_all, c_obs, shape: Sequence[int], origin, res: float, values_only: bool = False):
        """values_only: gto_set_scene_values, the fields without the solver's records and distance fields (such a scene
        serves plan_cost and eval_points only)."""
        ca = np.ascontiguousarray(c_all, dtype=np.float32).reshape(-1)
        co = None if c_obs is None else np.ascontiguousarray(c_obs, dtype=np.float32).reshape(-1)
        shp = _i32(list(shape))
        n = int(shp[0]) * int(shp[1]) * int(shp[2])
        if ca.size != n or (co is not None and co.size != n):
            raise ValueError(f"field size {ca.size} does not match shape {tuple(shp)}")
        org = _f64(np.asarray(origin).reshape(3))
        fn = self.lib.gto_set_scene_values if values_only else self.lib.gto_set_scene
        self._check(fn(self._h, scene_id, _p(ca, _pf), _p(co, _pf), _p(shp, _pi), _p(org, _pd), float(res)),
                    "gto_set_scene_values" if values_only else "gto_set_scene")
        self.scenes[scene_id] = (tuple(int(s) for s in shp), org.copy(), float(res))
        self._bump(scene_id)

    def _bump(self, scene_id: int):
        """A scene of this handle was written: handles that borrowed it (share_scene) hold pointers into buffers that are
        gone.  Borrowers remember the generation they shared and share again when it has moved (scene_generation)."""
        self._scene_gen[int(scene_id)] = self._scene_gen.get(int(scene_id), 0) + 1

    def scene_generation(self, scene_id: int) -> int:
        return self._scene_gen.get(int(scene_id), 0)

    def scene_from_depth(self, scene_id: int, depth, K, cam_pose, target_mask=None, threshold=1.5, grid_res=0.05, margin=0.4,
                         epsilon=0.02, w_inside=1.0, depth_obstacle=None):
        """gto_scene_from_depth: depth image -> both cost fields resident as scene `scene_id` (voxel records and distance
        fields included); returns (shape, origin, bounds (3, 2)) of the grid, nothing else leaves the device.
        depth_obstacle: the image of the second cloud (the driver's copy with the target's pixels at the threshold,
        examples/pybullet_gto_planning.py:187-189); None: the same image."""
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        Hh, Ww = depth.shape
        dobs = None if depth_obstacle is None else np.ascontiguousarray(depth_obstacle, dtype=np.float32)
        if dobs is not None and dobs.shape != depth.shape:
            raise ValueError("depth_obstacle must have the shape of depth")
        K = _f64(K).reshape(3, 3)
        cam = _f64(cam_pose).reshape(4, 4)
        Kinv, cinv = np.ascontiguousarray(np.linalg.inv(K)), np.ascontiguousarray(np.linalg.inv(cam))
        mask = None if target_mask is None else np.ascontiguousarray(target_mask, dtype=np.uint8)
        shp, org, bnd = np.zeros(3, np.int32), np.zeros(3), np.zeros(6)
        pu8 = C.POINTER(C.c_uint8)
        self._check(self.lib.gto_scene_from_depth(self._h, scene_id, _p(depth, _pf), Hh, Ww, _p(K, _pd), _p(Kinv, _pd), _p(cam, _pd), _p(cinv, _pd),
                                                  None if mask is None else mask.ctypes.data_as(pu8), _p(dobs, _pf), float(threshold), float(grid_res), float(margin),
                                                  float(epsilon), float(w_inside), _p(shp, _pi), _p(org, _pd), _p(bnd, _pd)), "gto_scene_from_depth")
        self.scenes[scene_id] = (tuple(int(x) for x in shp), org.copy(), float(grid_res))
        self._bump(scene_id)
        return tuple(int(x) for x in shp), org, np.stack((bnd[:3], bnd[3:]), axis=1)

    def scene_from_clouds(self, scene_id: int, points, normals, n_obstacle=None, k=11, grid_res=0.05, margin=0.4, epsilon=0.02,
                          w_inside=1.0):
        """gto_scene_from_clouds: sampled meshes -> both cost fields resident as scene `scene_id`; the first `n_obstacle`
        samples are the scene without the target object (None: all of them, one field used twice).  Returns (shape, origin,
        bounds (3, 2)) of the grid, nothing else leaves the device."""
        pts, nrm = _f64(points).reshape(-1, 3), _f64(normals).reshape(-1, 3)
        if pts.shape != nrm.shape:
            raise ValueError("points and normals must have the same shape")
        n_all = pts.shape[0]
        shp, org, bnd = np.zeros(3, np.int32), np.zeros(3), np.zeros(6)
        self._check(self.lib.gto_scene_from_clouds(self._h, scene_id, _p(pts, _pd), _p(nrm, _pd), n_all, n_all if n_obstacle is None else int(n_obstacle),
                                                   int(k), float(grid_res), float(margin), float(epsilon), float(w_inside), _p(shp, _pi), _p(org, _pd),
                                                   _p(bnd, _pd)), "gto_scene_from_clouds")
        self.scenes[scene_id] = (tuple(int(x) for x in shp), org.copy(), float(grid_res))
        self._bump(scene_id)
        return tuple(int(x) for x in shp), org, np.stack((bnd[:3], bnd[3:]), axis=1)

    def scene_fields(self, scene_id: int):
        """(c_all, c_obs) of a resident scene as float32 arrays (device to host)."""
        shape = self.scenes[scene_id][0]
        n = int(np.prod(shape))
        ca, co = np.empty(n, np.float32), np.empty(n, np.float32)
        self._check(self.lib.gto_get_scene_fields(self._h, scene_id, _p(ca, _pf), _p(co, _pf)), "gto_get_scene_fields")
        return ca, co

    def drop_scene(self, scene_id: int):
        self._check(self.lib.gto_drop_scene(self._h, scene_id), "gto_drop_scene")
        self.scenes.pop(scene_id, None)
        self._bump(scene_id)

    # -------------------------------------------------------------- solve
    def solve_batch(self, scene_id, qc, goals, n_goals, standoff, base_pos, Q0, out=None):
        """gto_solve_batch through host arrays.  ``out``: optional tuple (Q, dQ, cost, iters, status) of C-contiguous arrays
        to write into (shapes (B,ndof,T) f64, (B,ndof,T-1) f64, (B,) f64, (B,) i32, (B,) i32): a caller that solves batch
        after batch keeps its result arrays instead of having fresh pages mapped and faulted in on every call."""
        d, T = self.desc, self.T
        qc = _f64(qc).reshape(-1, d.ndof)
        B = qc.shape[0]
        if B == 0:  # empty batch: nothing to solve
            return (np.empty((0, d.ndof, T)), np.empty((0, d.ndof, T - 1)), np.empty(0),
                    np.empty(0, dtype=np.int32), np.empty(0, dtype=np.int32))
        goals = _f64(goals).reshape(B, -1, 16)
        n_max = goals.shape[1]
        n_goals = _per_instance(n_goals, B)
        scene_id = _per_instance(scene_id, B)
        so = None if standoff is None else _f64(np.broadcast_to(_f64(standoff).reshape(-1, 16), (B, 16)))
        base = _bases(base_pos, B)
        Q0 = _f64(Q0).reshape(B, d.ndof, T)
        if out is not None:
            Q, dQ, cost, iters, status = out
            want = (((B, d.ndof, T), np.float64), ((B, d.ndof, T - 1), np.float64), ((B,), np.float64), ((B,), np.int32), ((B,), np.int32))
            for a, (shp, dt) in zip(out, want):
                if a.shape != shp or a.dtype != dt or not a.flags.c_contiguous:
                    raise ValueError(f"solve_batch(out=): expected a C-contiguous {np.dtype(dt).name} array of shape {shp}, got {a.dtype} {a.shape}")
        else:
            Q = np.empty((B, d.ndof, T))
            dQ = np.empty((B, d.ndof, T - 1))
            cost = np.empty(B)
            iters = np.empty(B, dtype=np.int32)
            status = np.empty(B, dtype=np.int32)
        arrays = (scene_id, qc, goals, n_goals, so, base, Q0, Q, dQ, cost, iters, status)
        rc = self.lib.gto_solve_batch(self._h, B, n_max, *(_p(a, C.c_void_p) for a in arrays))
        self._check(rc, "gto_solve_batch")
        return Q, dQ, cost, iters, status

    def solve_batch_device(self, B, n_max, scene_id, qc, goals, n_goals, standoff, base_pos, Q0,
                           Q_out, dQ_out, cost_out, iters_out, status_out, stream=None):
        """All arguments are device pointers (ints, e.g. torch.Tensor.data_ptr()) or None."""
        rc = self.lib.gto_solve_batch_device(self._h, B, n_max, _vp(scene_id), _vp(qc), _vp(goals), _vp(n_goals),
                                             _vp(standoff), _vp(base_pos), _vp(Q0), _vp(Q_out), _vp(dQ_out),
                                             _vp(cost_out), _vp(iters_out), _vp(status_out), _vp(stream))
        self._check(rc, "gto_solve_batch_device")

    def share_scene(self, scene_id, src: "SolverHandle", src_scene_id=None, all_from: int = 0, obs_from: int = 1):
        """Use a scene that lives in another handle on the same GPU without a second copy.  all_from / obs_from: which of
        the source's two fields (0: sdf_cost_all, 1: sdf_cost_obstacle) this handle sees as its sdf_cost_all / sdf_cost_obstacle
        (gto_share_scene_halves)."""
        src_id = int(scene_id if src_scene_id is None else src_scene_id)
        if (all_from, obs_from) == (0, 1):
            self._check(self.lib.gto_share_scene(self._h, int(scene_id), src._h, src_id), "gto_share_scene")
        else:
            self._check(self.lib.gto_share_scene_halves(self._h, int(scene_id), src._h, src_id, int(all_from), int(obs_from)), "gto_share_scene_halves")
        if src_id in src.scenes:
            self.scenes[int(scene_id)] = src.scenes[src_id]
        self._bump(scene_id)

    def set_stream(self, stream):
        """Bind every launch/copy of this handle to the caller's HIP stream (an int such as
        torch.cuda.Stream.cuda_stream); None restores a private stream."""
        self._check(self.lib.gto_set_stream(self._h, _vp(stream)), "gto_set_stream")

    MODE_ROUNDS, MODE_SINGLE_LAUNCH = 0, 1

    def set_mode(self, mode: int):
        """MODE_ROUNDS (default): evaluate / step launches over slots; MODE_SINGLE_LAUNCH: one launch per call."""
        self._check(self.lib.gto_set_mode(self._h, int(mode)), "gto_set_mode")

    def set_lanes(self, max_lanes: int = 1, min_per_lane: int = 256, adopt_below: int = 0):
        """Lanes of a solve call (include/gto_solver.h, gto_set_lanes): streams the call's instances are dealt to, one host
        thread of the call each.  The defaults are the library's (one lane: no thread but the caller's): several lanes are
        asked for explicitly, e.g. set_lanes(4, 256, 0)."""
        self._check(self.lib.gto_set_lanes(self._h, int(max_lanes), int(min_per_lane), int(adopt_below)), "gto_set_lanes")

    def set_lane_streams(self, streams=()):
        """The lanes' HIP streams (raw handles, e.g. torch.cuda.Stream(...).cuda_stream); () = the handle's own."""
        arr = (C.c_void_p * max(1, len(streams)))(*[C.c_void_p(int(x)) for x in streams])
        self._check(self.lib.gto_set_lane_streams(self._h, len(streams), arr), "gto_set_lane_streams")

    def set_profiling(self, enabled: bool):
        self._check(self.lib.gto_set_profiling(self._h, int(enabled)), "gto_set_profiling")

    def last_kernel_time(self):
        ms = C.c_double()
        n = C.c_int32()
        self._check(self.lib.gto_last_kernel_time(self._h, C.byref(ms), C.byref(n)), "gto_last_kernel_time")
        return ms.value, n.value

    def last_kernel_work(self):
        """(surface points gathered, chunk spheres tested) by the dominant kernel during the last profiled solve."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.lib.gto_last_kernel_work(self._h, C.byref(a), C.byref(b)), "gto_last_kernel_work")
        return a.value, b.value

    PROF_VARIANTS = ("k_obstacle_gram<8,1>", "k_obstacle_gram<8,8>", "k_lm_step<4,1>", "k_lm_step<8,4>")

    def last_kernel_profile(self):
        """Per kernel variant of the last profiled solve: {name: (ms, launches, workgroups, points gathered)}."""
        out = {}
        names = self.PROF_VARIANTS
        if self.desc.n_opt > 8:  # the kernels of the robots with nine to sixteen optimised joints (one step kernel, no few-instance variants)
            names = ("k_obstacle_gram<16,1>", "k_obstacle_gram<16,8>", "k_lm_step_wide<16>", "k_lm_step<8,4>")
        for v, name in enumerate(names):
            ms, n, wg, pts = C.c_double(), C.c_int32(), C.c_uint64(), C.c_uint64()
            self._check(self.lib.gto_last_kernel_profile(self._h, v, C.byref(ms), C.byref(n), C.byref(wg), C.byref(pts)), "gto_last_kernel_profile")
            out[name] = (ms.value, n.value, wg.value, pts.value)
        return out

    def last_seed_test_profile(self):
        """(ms, launches, workgroups) of k_seed_broad in the last profiled solve: the seeds of the instances that waited for a
        slot, tested against the distance field once per call (no launch: the call had no such instance, or no broad phase)."""
        ms, n, wg, pts = C.c_double(), C.c_int32(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.gto_last_kernel_profile(self._h, 4, C.byref(ms), C.byref(n), C.byref(wg), C.byref(pts)), "gto_last_kernel_profile")
        return ms.value, n.value, wg.value

    # -------------------------------------------------------------- evaluation entry points
    def eval_fk(self, q):
        q = _f64(q).reshape(-1, self.desc.ndof)
        out = np.empty((q.shape[0], self.desc.n_frames, 4, 4))
        self._check(self.lib.gto_eval_fk(self._h, q.shape[0], _p(q, _pd), _p(out, _pd)), "gto_eval_fk")
        return out

    def set_link_inertials(self, mass, com, inertia, gravity=None):
        """The inertials of the handle's frames (gto_set_link_inertials): mass (F,), com (F, 3), inertia (F, 6) as
        ixx ixy ixz iyy iyz izz about the centre of mass in the frame's axes; gravity (3,) in the base frame, None =
        (0, 0, -9.81)."""
        F = self.desc.n_frames
        mass, com, inertia = _f64(mass).reshape(-1), _f64(com).reshape(-1), _f64(inertia).reshape(-1)
        if mass.size != F or com.size != 3 * F or inertia.size != 6 * F:
            raise ValueError(f"set_link_inertials: mass ({F},), com ({F}, 3) and inertia ({F}, 6) expected")
        g = None if gravity is None else _f64(gravity).reshape(3)
        self._check(self.lib.gto_set_link_inertials(self._h, _p(mass, _pd), _p(com, _pd), _p(inertia, _pd), _p(g, _pd)),
                    "gto_set_link_inertials")

    def sync_link_inertials(self):
        """Upload the description's inertials if it has any and they are not the arrays this handle uploaded last (a
        description loaded from the packaged files has none until RobotDesc.set_link_inertials)."""
        d = self.desc
        if d.has_inertials and (self._inertials is None or any(a is not b for a, b in zip(
                self._inertials, (d.frame_mass, d.frame_com, d.frame_inertia)))):
            self.set_link_inertials(d.frame_mass, d.frame_com, d.frame_inertia)
            self._inertials = (d.frame_mass, d.frame_com, d.frame_inertia)

    def inverse_dynamics(self, q, qd, qdd, payload=None):
        """Joint forces (n, ndof) of the rows q, qd, qdd (n, ndof) by gto_inverse_dynamics.  payload: None, or a dict with
        "mass" and optionally "com" (in link_ee's frame) and "inertia" (ixx ixy ixz iyy iyz izz about that centre), each
        one value for the call or one per row."""
        q = _f64(q).reshape(-1, self.desc.ndof)
        n = q.shape[0]
        qd, qdd = _f64(qd).reshape(n, self.desc.ndof), _f64(qdd).reshape(n, self.desc.ndof)
        pm, pc, pi = payload_arrays(payload, n)
        self.sync_link_inertials()
        out = np.empty((n, self.desc.ndof))
        self._check(self.lib.gto_inverse_dynamics(self._h, n, _p(q, _pd), _p(qd, _pd), _p(qdd, _pd), _p(pm, _pd), _p(pc, _pd),
                                                  _p(pi, _pd), _p(out, _pd)), "gto_inverse_dynamics")
        return out

    def forward_dynamics(self, q, qd, tau, payload=None, locked=None, want_mass_matrix=False):
        """Accelerations (n, ndof) that the joint forces tau cause at the rows q, qd (n, ndof), by gto_forward_dynamics, and
        the status (n,) of every row (2: a non-finite row or a free joint that moves no mass, NaN there).  payload: the dict
        of inverse_dynamics.  locked: None (every joint that is not optimised stands still) or one flag per joint.  Returns
        (qdd, status), and the symmetrised mass matrix (n, ndof, ndof) as a third entry with want_mass_matrix."""
        nd = self.desc.ndof
        q = _f64(q).reshape(-1, nd)
        n = q.shape[0]
        qd, tau = _f64(qd).reshape(n, nd), _f64(tau).reshape(n, nd)
        pm, pc, pi = payload_arrays(payload, n)
        lk = None
        if locked is not None:
            lk = np.asarray(locked)
            if lk.shape != (nd,):
                raise ValueError(f"forward_dynamics: locked must be ({nd},), got shape {lk.shape}")
            lk = _i32(lk != 0)
        self.sync_link_inertials()
        qdd, status = np.empty((n, nd)), np.empty(n, dtype=np.int32)
        Mm = np.empty((n, nd, nd)) if want_mass_matrix else None
        self._check(self.lib.gto_forward_dynamics(self._h, n, _p(q, _pd), _p(qd, _pd), _p(tau, _pd), _p(pm, _pd), _p(pc, _pd),
                                                  _p(pi, _pd), _p(lk, _pi), _p(qdd, _pd), _p(Mm, _pd), _p(status, _pi)),
                    "gto_forward_dynamics")
        return (qdd, status, Mm) if want_mass_matrix else (qdd, status)

    def track_rollout(self, duration, q_ref, qd_ref, qdd_ref, kp, kd, tau_max=None, dt=1e-3, settle=0.0, n_samples=100,
                      feedforward="full", model_payload=None, plant_payload=None, locked=None):
        """gto_track_rollout: roll the B references (duration (B,), samples (B, M, ndof) at linspace(0, duration, M)) forward
        under tau = clip(ff + kp (q_ref - q) + kd (qd_ref - qd), +-tau_max), evaluated every ``dt`` and held, on the plant
        with ``plant_payload`` in the hand while the feedforward believes ``model_payload`` (each the dict of
        inverse_dynamics, one value for the call or one per path).  Returns a dict: q, qd (B, n_samples, ndof), t
        (B, n_samples), err_max, err_end (B,), sat_steps, steps, status (B,) int32."""
        d = self.desc
        q_ref = _f64(q_ref)
        if q_ref.ndim != 3 or q_ref.shape[2] != d.ndof:
            raise ValueError(f"track_rollout: q_ref must be (B, M, {d.ndof}), got {q_ref.shape}")
        B, M = q_ref.shape[:2]
        qd_ref, qdd_ref = _f64(qd_ref).reshape(q_ref.shape), _f64(qdd_ref).reshape(q_ref.shape)
        duration = _f64(duration).reshape(B)
        kp, kd, tm, dt, settle, Mo, ff, lk = track_controller(d, kp, kd, tau_max, dt, settle, n_samples, feedforward, locked, need_inertials=False)
        mm, mc, mi = payload_arrays(model_payload, B)
        pm, pc, pi = payload_arrays(plant_payload, B)
        self.sync_link_inertials()
        out = dict(q=np.empty((B, Mo, d.ndof)), qd=np.empty((B, Mo, d.ndof)), t=np.empty((B, Mo)), err_max=np.empty(B),
                   err_end=np.empty(B), sat_steps=np.empty(B, dtype=np.int32), steps=np.empty(B, dtype=np.int32),
                   status=np.empty(B, dtype=np.int32))
        self._check(self.lib.gto_track_rollout(self._h, B, M, _p(duration, _pd), _p(q_ref, _pd), _p(qd_ref, _pd), _p(qdd_ref, _pd),
                                               _p(kp, _pd), _p(kd, _pd), _p(tm, _pd), dt, settle, ff, _p(mm, _pd), _p(mc, _pd),
                                               _p(mi, _pd), _p(pm, _pd), _p(pc, _pd), _p(pi, _pd), _p(lk, _pi), Mo,
                                               _p(out["q"], _pd), _p(out["qd"], _pd), _p(out["t"], _pd), _p(out["err_max"], _pd),
                                               _p(out["err_end"], _pd), _p(out["sat_steps"], _pi), _p(out["steps"], _pi),
                                               _p(out["status"], _pi)), "gto_track_rollout")
        return out

    def track_rollout_device(self, B, M, duration, q_ref, qd_ref, qdd_ref, kp, kd, tau_max=None, dt=1e-3, settle=0.0,
                             n_samples=100, feedforward="full", model_payload=(None, None, None),
                             plant_payload=(None, None, None), locked=None, q_out=None, qd_out=None, t_out=None, err_max=None,
                             err_end=None, sat_steps=None, steps=None, status_out=None, stream=None):
        """gto_track_rollout_device: duration (B,), the samples (B, M, ndof), the payloads ((mass (B,), com (B, 3), inertia
        (B, 6)) each, any of them None) and the outputs are device pointers (ints, e.g. torch.Tensor.data_ptr()) or None;
        the gains, limits, clock and ``locked`` are host values.  One launch on ``stream``, nothing else."""
        kp, kd, tm, dt, settle, Mo, ff, lk = track_controller(self.desc, kp, kd, tau_max, dt, settle, n_samples, feedforward, locked,
                                                              need_inertials=False)
        self.sync_link_inertials()
        self._check(self.lib.gto_track_rollout_device(self._h, int(B), int(M), _vp(duration), _vp(q_ref), _vp(qd_ref), _vp(qdd_ref),
                                                      _p(kp, _pd), _p(kd, _pd), _p(tm, _pd), dt, settle, ff,
                                                      *[_vp(a) for a in tuple(model_payload) + tuple(plant_payload)], _p(lk, _pi), Mo,
                                                      _vp(q_out), _vp(qd_out), _vp(t_out), _vp(err_max), _vp(err_end),
                                                      _vp(sat_steps), _vp(steps), _vp(status_out), _vp(stream)),
                    "gto_track_rollout_device")

    def eval_points(self, scene_id, q, base_pos, use_obs=False, want_field=True, want=None):
        """World surface points, voxel offsets, field values and field gradients of configurations q (nq, ndof).
        ``want``: the outputs to bring back, any of "xyz", "off", "val", "grad" (default: all, or xyz alone with
        want_field=False); the others are None and cost neither device memory nor a transfer."""
        q = _f64(q).reshape(-1, self.desc.ndof)
        nq, P = q.shape[0], self.desc.n_points
        base = _bases(base_pos, nq)
        if want is None:
            want = ("xyz", "off", "val", "grad") if want_field else ("xyz",)
        xyz = np.empty((nq, P, 3)) if "xyz" in want else None
        off = np.empty((nq, P), dtype=np.int32) if "off" in want else None
        val = np.empty((nq, P)) if "val" in want else None
        grad = np.empty((nq, P, 3)) if "grad" in want else None
        self._check(self.lib.gto_eval_points(self._h, scene_id, nq, _p(q, _pd), _p(base, _pd), int(use_obs),
                                             _p(xyz, _pd), _p(off, _pi), _p(val, _pd), _p(grad, _pd)),
                    "gto_eval_points")
        return xyz, off, val, grad

    def eval_points_hessian(self, scene_id, q, base_pos, use_obs=False):
        """Hessian of the selected cost field at the surface points of configurations q: (nq, P, 3, 3), gto/sdf_callback.py:165-183."""
        q = _f64(q).reshape(-1, self.desc.ndof)
        nq, P = q.shape[0], self.desc.n_points
        base = _bases(base_pos, nq)
        out = np.empty((nq, P, 3, 3))
        self._check(self.lib.gto_eval_points_hessian(self._h, scene_id, nq, _p(q, _pd), _p(base, _pd), int(use_obs), _p(out, _pd)), "gto_eval_points_hessian")
        return out

    def eval_objective(self, scene_id, goals, n_goals, standoff, base_pos, Q):
        d, T = self.desc, self.T
        Q = _f64(Q).reshape(-1, d.ndof, T)
        B = Q.shape[0]
        goals = _f64(goals).reshape(B, -1, 16)
        n_max = goals.shape[1]
        n_goals = _per_instance(n_goals, B)
        scene_id = _per_instance(scene_id, B)
        so = None if standoff is None else _f64(np.broadcast_to(_f64(standoff).reshape(-1, 16), (B, 16)))
        base = _bases(base_pos, B)
        fg, fo, fv = np.empty(B), np.empty(B), np.empty(B)
        am = np.empty(B, dtype=np.int32)
        self._check(self.lib.gto_eval_objective(self._h, B, n_max, _p(scene_id, _pi), _p(goals, _pd),
                                                _p(n_goals, _pi), _p(so, _pd), _p(base, _pd), _p(Q, _pd),
                                                _p(fg, _pd), _p(fo, _pd), _p(fv, _pd), _p(am, _pi)),
                    "gto_eval_objective")
        return fg, fo, fv, am

    def eval_obstacle_normal_eq(self, scene_id, base_pos, Q):
        d, T, n = self.desc, self.T, self.desc.n_opt
        Q = _f64(Q).reshape(-1, d.ndof, T)
        B = Q.shape[0]
        scene_id = _per_instance(scene_id, B)
        base = _bases(base_pos, B)
        JtJ, Jtr, ss = np.empty((B, T, n, n)), np.empty((B, T, n)), np.empty((B, T))
        self._check(self.lib.gto_eval_obstacle_normal_eq(self._h, B, _p(scene_id, _pi), _p(base, _pd),
                                                         _p(Q, _pd), _p(JtJ, _pd), _p(Jtr, _pd), _p(ss, _pd)),
                    "gto_eval_obstacle_normal_eq")
        return JtJ, Jtr, ss

    def solve_ik_batch(self, scene_id, q0, goals, base_pos=None, max_iter=50):
        """IK for B goal poses (gto/ik_solver.py:78-110); scene_id None = no collision term.
        Returns (q (B,ndof), cost (B,), iters (B,), status (B,))."""
        d = self.desc
        q0 = _f64(q0).reshape(-1, d.ndof)
        B = q0.shape[0]
        goals = _f64(goals).reshape(B, 16)
        sid = None if scene_id is None else _per_instance(scene_id, B)
        base = None if base_pos is None else _bases(base_pos, B)
        q, cost = np.empty((B, d.ndof)), np.empty(B)
        iters, status = np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
        if B:
            self._check(self.lib.gto_solve_ik_batch(self._h, B, _p(sid, _pi), _p(q0, _pd), _p(goals, _pd), _p(base, _pd),
                                                    int(max_iter), _p(q, _pd), _p(cost, _pd), _p(iters, _pi), _p(status, _pi)),
                        "gto_solve_ik_batch")
        return q, cost, iters, status

    IK_GOAL_WIDTH = {0: 16, 1: 7, 2: 6}  # GTO_IK_GOAL_POINTS / _QUATERNION / _RPY: doubles per goal

    def solve_ik_pose_batch(self, kind, scene_id, q0, goals, base_pos=None, max_iter=50):
        """IK for B goals of link_ee of one kind (include/gto_solver.h GTO_IK_GOAL_*): 0 = RT (B,16) as solve_ik_batch,
        1 = x y z qx qy qz qw (B,7) (gto/ik_solver_quaternion.py), 2 = x y z roll pitch yaw (B,6) (gto/ik_solver_rpy.py).
        Returns (q (B,ndof), cost (B,), iters (B,), status (B,))."""
        d = self.desc
        q0 = _f64(q0).reshape(-1, d.ndof)
        B = q0.shape[0]
        goals = _f64(goals).reshape(B, -1)
        if int(kind) in self.IK_GOAL_WIDTH and goals.shape[1] != self.IK_GOAL_WIDTH[int(kind)]:
            raise ValueError(f"goal kind {kind} takes {self.IK_GOAL_WIDTH[int(kind)]} numbers per goal, not {goals.shape[1]}")
        sid = None if scene_id is None else _per_instance(scene_id, B)
        base = None if base_pos is None else _bases(base_pos, B)
        q, cost = np.empty((B, d.ndof)), np.empty(B)
        iters, status = np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
        self._check(self.lib.gto_solve_ik_pose_batch(self._h, int(kind), B, _p(sid, _pi), _p(q0, _pd), _p(goals, _pd),
                                                     _p(base, _pd), int(max_iter), _p(q, _pd), _p(cost, _pd), _p(iters, _pi),
                                                     _p(status, _pi)),
                    "gto_solve_ik_pose_batch")
        return q, cost, iters, status

    # -------------------------------------------------------------- the stream-ordered chain (grasp_chain.GraspChain)
    def solve_ik_pose_batch_device(self, kind, B, scene_id, q0, goals, base_pos, max_iter, q_out, cost_out=None,
                                   iters_out=None, status_out=None, stream=None):
        """gto_solve_ik_pose_batch_device: all arrays are device pointers (ints, e.g. torch.Tensor.data_ptr()) or None;
        scene_id None = no collision term (base_pos may then be None)."""
        self._check(self.lib.gto_solve_ik_pose_batch_device(self._h, int(kind), int(B), _vp(scene_id), _vp(q0), _vp(goals),
                                                            _vp(base_pos), int(max_iter), _vp(q_out), _vp(cost_out), _vp(iters_out),
                                                            _vp(status_out), _vp(stream)), "gto_solve_ik_pose_batch_device")

    def ik_report_device(self, B, scene_id, q, goals, base_pos, pos_tol, rot_tol_deg, cost_tol, err_pos_out=None,
                         err_rot_out=None, cost_out=None, accept_out=None, stream=None):
        """gto_ik_report_device: err_pos, err_rot (degrees), collision cost and the acceptance flag (uint8) of B IK solutions;
        device pointers or None."""
        self._check(self.lib.gto_ik_report_device(self._h, int(B), _vp(scene_id), _vp(q), _vp(goals), _vp(base_pos), float(pos_tol),
                                                  float(rot_tol_deg), float(cost_tol), _vp(err_pos_out), _vp(err_rot_out),
                                                  _vp(cost_out), _vp(accept_out), _vp(stream)), "gto_ik_report_device")

    def seed_goalsets_device(self, B, n_max, scene_id, qc, goals, n_goals, q_solutions, accept, base_pos, interpolate,
                             solutions_f32, goals_out=None, n_goals_out=None, n_accepted_out=None, Q0_out=None,
                             seed_index_out=None, seed_cost_out=None, seed_dist_out=None, stream=None):
        """gto_seed_goalsets_device: accepted goal sets, seed scores, the chosen seed; device pointers or None."""
        self._check(self.lib.gto_seed_goalsets_device(self._h, int(B), int(n_max), _vp(scene_id), _vp(qc), _vp(goals), _vp(n_goals),
                                                      _vp(q_solutions), _vp(accept), _vp(base_pos), int(bool(interpolate)),
                                                      int(bool(solutions_f32)), _vp(goals_out), _vp(n_goals_out),
                                                      _vp(n_accepted_out), _vp(Q0_out), _vp(seed_index_out), _vp(seed_cost_out),
                                                      _vp(seed_dist_out), _vp(stream)), "gto_seed_goalsets_device")

    # -------------------------------------------------------------- several seeds per goal set (GraspChain.plan_objects(n_seeds=k))
    def seed_goalsets_multi_device(self, B, n_max, n_seeds, scene_id, qc, goals, n_goals, q_solutions, accept, base_pos, interpolate,
                                   solutions_f32, goals_out=None, n_goals_out=None, n_accepted_out=None, accepted_rows_out=None,
                                   Q0_out=None, seed_index_out=None, seed_cost_out=None, seed_dist_out=None, stream=None):
        """gto_seed_goalsets_multi_device: the n_seeds best seeds of every goal set, one slot of goals_out / n_goals_out /
        Q0_out / seed_index_out (leading shape (B, n_seeds)) each; device pointers or None."""
        self._check(self.lib.gto_seed_goalsets_multi_device(self._h, int(B), int(n_max), int(n_seeds), _vp(scene_id), _vp(qc), _vp(goals),
                                                            _vp(n_goals), _vp(q_solutions), _vp(accept), _vp(base_pos),
                                                            int(bool(interpolate)), int(bool(solutions_f32)), _vp(goals_out),
                                                            _vp(n_goals_out), _vp(n_accepted_out), _vp(accepted_rows_out), _vp(Q0_out),
                                                            _vp(seed_index_out), _vp(seed_cost_out), _vp(seed_dist_out), _vp(stream)),
                    "gto_seed_goalsets_multi_device")

    def plan_report_device(self, B, n_max, goals, n_goals, standoff, Q, goal_index_out=None, goal_cost_out=None, err_pos_out=None,
                           err_rot_out=None, stream=None):
        """gto_plan_report_device: the goal every plan reached (the objective's arg-min goal), that goal's term and err_pos /
        err_rot (degrees) of the last waypoint against it; device pointers or None."""
        self._check(self.lib.gto_plan_report_device(self._h, int(B), int(n_max), _vp(goals), _vp(n_goals), _vp(standoff), _vp(Q),
                                                    _vp(goal_index_out), _vp(goal_cost_out), _vp(err_pos_out), _vp(err_rot_out),
                                                    _vp(stream)), "gto_plan_report_device")

    def select_plans_device(self, B, n_seeds, status, cost, err_pos, err_rot, counts, pos_tol, rot_tol_deg, max_points, Q=None,
                            dQ=None, best_slot_out=None, class_out=None, Q_out=None, dQ_out=None, stream=None):
        """gto_select_plans_device: the class of every slot's plan and the best slot of every object, with copies of its
        rows; device pointers or None."""
        self._check(self.lib.gto_select_plans_device(self._h, int(B), int(n_seeds), _vp(status), _vp(cost), _vp(err_pos), _vp(err_rot),
                                                     _vp(counts), float(pos_tol), float(rot_tol_deg), int(max_points), _vp(Q), _vp(dQ),
                                                     _vp(best_slot_out), _vp(class_out), _vp(Q_out), _vp(dQ_out), _vp(stream)),
                    "gto_select_plans_device")

    # -------------------------------------------------------------- the grasp collision filter (GraspChain.plan_grasps)
    def filter_grasps_device(self, observations, n_max, points, P, object_pose, grasps, n_grasps, check_offset, ik_offset=None,
                             world_to_base=None, base_pos=None, max_ratio=0.01, count_out=None, keep_out=None, kept_rows_out=None,
                             n_kept_out=None, n_grasps_out=None, plan_goals_out=None, ik_goals_out=None, stream=None):
        """gto_filter_grasps_device: observations is a HOST sequence of observation.Observation, one per object (B = its
        length; entries may repeat); check_offset and ik_offset are HOST 4x4 matrices; every other array is a device
        pointer (an int, e.g. torch.Tensor.data_ptr()) or None."""
        B = len(observations)
        obs = (C.c_void_p * max(1, B))(*[o._ptr() for o in observations])
        co = _f64(check_offset).reshape(16)
        io = None if ik_offset is None else _f64(ik_offset).reshape(16)
        self._check(self.lib.gto_filter_grasps_device(self._h, B, int(n_max), obs, _vp(points), int(P), _vp(object_pose), _vp(grasps),
                                                      _vp(n_grasps), _vp(world_to_base), _vp(base_pos), _p(co, _pd), _p(io, _pd),
                                                      float(max_ratio), _vp(count_out), _vp(keep_out), _vp(kept_rows_out),
                                                      _vp(n_kept_out), _vp(n_grasps_out), _vp(plan_goals_out), _vp(ik_goals_out),
                                                      _vp(stream)), "gto_filter_grasps_device")

    def solve_base_batch(self, qc, goals, n_goals=None, effort_weight=0.01, max_iter=100):
        """Base placement for B goal sets (gto/base_planner.py:35-123): qc (B,ndof), goals (B,n_max,4,4).
        Returns (y (B,3) = x, y, theta, q (B,n_max,ndof), cost (B,), iters (B,), status (B,))."""
        d = self.desc
        qc = _f64(qc).reshape(-1, d.ndof)
        B = qc.shape[0]
        goals = _f64(goals).reshape(B, -1, 16)
        n_max = goals.shape[1]
        ng = _per_instance(n_max if n_goals is None else n_goals, B)
        y, q, cost = np.empty((B, 3)), np.empty((B, n_max, d.ndof)), np.empty(B)
        iters, status = np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
        if B:
            self._check(self.lib.gto_solve_base_batch(self._h, B, n_max, _p(ng, _pi), _p(qc, _pd), _p(goals, _pd),
                                                      float(effort_weight), int(max_iter), _p(y, _pd), _p(q, _pd),
                                                      _p(cost, _pd), _p(iters, _pi), _p(status, _pi)),
                        "gto_solve_base_batch")
        return y, q, cost, iters, status

    # -------------------------------------------------------------- the stream-ordered base placement (BasePlanner.place_base)
    def solve_base_batch_device(self, B, n_max, n_goals, qc, goals, effort_weight, max_iter, y_out, q_out, cost_out=None,
                                iters_out=None, status_out=None, stream=None):
        """gto_solve_base_batch_device: n_goals is a HOST int32 array (B,); every other array is a device pointer (an int,
        e.g. torch.Tensor.data_ptr()) or None."""
        ng = _per_instance(n_goals, int(B))
        self._check(self.lib.gto_solve_base_batch_device(self._h, int(B), int(n_max), _p(ng, _pi), _vp(qc), _vp(goals),
                                                         float(effort_weight), int(max_iter), _vp(y_out), _vp(q_out), _vp(cost_out),
                                                         _vp(iters_out), _vp(status_out), _vp(stream)), "gto_solve_base_batch_device")

    def base_report_device(self, occ, B, n_max, n_goals, qc, goals, y, q, err_pos_out=None, err_rot_out=None,
                           collision_out=None, first_free_out=None, stream=None):
        """gto_base_report_device: err_pos / err_rot (degrees) of every goal, the footprint count of every set on the
        occupancy grid ``occ`` (occupancy.OccupancyGrid or None) and the first free set; n_goals is a HOST array, the others
        device pointers or None."""
        ng = _per_instance(n_goals, int(B))
        self._check(self.lib.gto_base_report_device(self._h, None if occ is None else occ._ptr(), int(B), int(n_max), _p(ng, _pi),
                                                    _vp(qc), _vp(goals), _vp(y), _vp(q), _vp(err_pos_out), _vp(err_rot_out),
                                                    _vp(collision_out), _vp(first_free_out), _vp(stream)), "gto_base_report_device")

    def eval_base_objective(self, y, q, goals, n_goals=None, effort_weight=0.01):
        """Base-placement objective (gto/base_planner.py:57-87) at y (B,3), q (B,n_max,ndof), goals (B,n_max,4,4)."""
        d = self.desc
        y = _f64(y).reshape(-1, 3)
        B = y.shape[0]
        goals = _f64(goals).reshape(B, -1, 16)
        n_max = goals.shape[1]
        q = _f64(q).reshape(B, n_max, d.ndof)
        ng = _per_instance(n_max if n_goals is None else n_goals, B)
        cost = np.empty(B)
        if B:
            self._check(self.lib.gto_eval_base_objective(self._h, B, n_max, _p(ng, _pi), _p(y, _pd), _p(q, _pd), _p(goals, _pd),
                                                         float(effort_weight), _p(cost, _pd)), "gto_eval_base_objective")
        return cost

    def plan_cost(self, scene_id, plans, base_pos):
        d, T = self.desc, self.T
        plans = _f64(plans).reshape(-1, d.ndof, T)
        n = plans.shape[0]
        base = _f64(np.asarray(base_pos).reshape(3))
        cost, dist = np.empty(n), np.empty(n)
        self._check(self.lib.gto_plan_cost(self._h, scene_id, n, _p(plans, _pd), _p(base, _pd),
                                           _p(cost, _pd), _p(dist, _pd)), "gto_plan_cost")
        return cost, dist

    # -------------------------------------------------------------- collision checks against a resident observation
    def _check_base(self, base_pos, B):
        """(host array, per_plan flag) of a base position (3,) or per-plan bases (B, 3)."""
        base = _f64(base_pos)
        if base.shape == (3,):
            return base, 0
        if base.shape != (B, 3):
            raise GTOError(f"check_plans: base_pos must be (3,) or ({B}, 3), one base per plan; got {base.shape}")
        return base, 1

    def check_plans(self, obs, plans, base_pos=(0.0, 0.0, 0.0)):
        """gto_check_plans: for plans (B, ndof, T) the number of the robot's surface points inside the observation ``obs``
        (observation.Observation) at every waypoint, int32 (B, T); -1 where a waypoint holds a non-finite entry.
        base_pos (3,) for all plans or (B, 3)."""
        d, T = self.desc, self.T
        plans = _f64(plans)
        if plans.ndim != 3 or plans.shape[1:] != (d.ndof, T):
            raise GTOError(f"check_plans: plans must have shape (B, {d.ndof}, {T}) -- ndof joints by the handle's horizon T = {T} "
                           f"waypoints -- got {plans.shape}")
        B = plans.shape[0]
        base, per_plan = self._check_base(base_pos, B)
        count = np.empty((B, T), dtype=np.int32)
        self._check(self.lib.gto_check_plans(self._h, obs._ptr(), B, _p(plans, _pd), _p(base, _pd), per_plan, _p(count, _pi)),
                    "gto_check_plans")
        return count

    def check_plans_device(self, obs, B, plans, count_out, base_pos=(0.0, 0.0, 0.0), stream=None):
        """gto_check_plans_device: plans (B, ndof, T) float64 and count_out (B, T) int32 are device pointers (ints, e.g.
        torch.Tensor.data_ptr()); enqueued on ``stream`` (None: the handle's) without a host synchronisation."""
        base, per_plan = self._check_base(base_pos, int(B))
        self._check(self.lib.gto_check_plans_device(self._h, obs._ptr(), int(B), _vp(plans), _p(base, _pd), per_plan, _vp(count_out),
                                                    _vp(stream)), "gto_check_plans_device")

    def check_paths(self, obs, paths, base_pos=(0.0, 0.0, 0.0)):
        """gto_check_paths: check_plans for paths (B, ndof, Tp) of any length Tp >= 1; int32 (B, Tp)."""
        paths = _f64(paths)
        if paths.ndim != 3 or paths.shape[1] != self.desc.ndof or paths.shape[2] < 1:
            raise GTOError(f"check_paths: paths must have shape (B, {self.desc.ndof}, Tp >= 1); got {paths.shape}")
        B, Tp = paths.shape[0], paths.shape[2]
        base, per_plan = self._check_base(base_pos, B)
        count = np.empty((B, Tp), dtype=np.int32)
        self._check(self.lib.gto_check_paths(self._h, obs._ptr(), B, Tp, _p(paths, _pd), _p(base, _pd), per_plan, _p(count, _pi)),
                    "gto_check_paths")
        return count

    def check_paths_device(self, obs, B, Tp, paths, count_out, base_pos=(0.0, 0.0, 0.0), stream=None):
        """gto_check_paths_device: check_plans_device with the number of columns Tp given: paths (B, ndof, Tp) float64 and
        count_out (B, Tp) int32 are device pointers."""
        base, per_plan = self._check_base(base_pos, int(B))
        self._check(self.lib.gto_check_paths_device(self._h, obs._ptr(), int(B), int(Tp), _vp(paths), _p(base, _pd), per_plan,
                                                    _vp(count_out), _vp(stream)), "gto_check_paths_device")

    def set_self_pairs(self, mask):
        """gto_set_self_pairs: the link pairs self_clearance compares, an (L, L) bool array, symmetric with a false
        diagonal (RobotDesc.self_pairs builds one); None: back to every pair of distinct links, what a new handle uses."""
        if mask is None:
            self._check(self.lib.gto_set_self_pairs(self._h, None), "gto_set_self_pairs")
            return
        rows = self_pair_rows(mask, self.desc.n_links)
        self._check(self.lib.gto_set_self_pairs(self._h, _p(rows, _pi)), "gto_set_self_pairs")

    def self_clearance(self, paths, cutoff=np.inf):
        """gto_self_clearance: for paths (B, ndof, Tp) the robot's smallest distance from itself at every column, over the
        pairs of set_self_pairs.  Returns a dict: d2 (B, Tp) float64 squared metres, min(d2, cutoff^2); pair (B, Tp, 2) int32
        the closest link pair (a < b), (-1, -1) where nothing is closer than the cutoff; dist = sqrt(d2).  A column with a
        non-finite entry: NaN and (-1, -1)."""
        paths = _f64(paths)
        if paths.ndim != 3 or paths.shape[1] != self.desc.ndof or paths.shape[2] < 1:
            raise GTOError(f"self_clearance: paths must have shape (B, {self.desc.ndof}, Tp >= 1); got {paths.shape}")
        B, Tp = paths.shape[0], paths.shape[2]
        d2, pair = np.empty((B, Tp)), np.empty((B, Tp, 2), dtype=np.int32)
        self._check(self.lib.gto_self_clearance(self._h, B, Tp, _p(paths, _pd), float(cutoff), _p(d2, _pd), _p(pair, _pi)),
                    "gto_self_clearance")
        return dict(d2=d2, pair=pair, dist=np.sqrt(d2))

    def self_clearance_device(self, B, Tp, paths, d2_out, pair_out, cutoff=np.inf, stream=None):
        """gto_self_clearance_device: paths (B, ndof, Tp) float64, d2_out (B, Tp) float64 and pair_out (B, Tp, 2) int32 are
        device pointers (ints, e.g. torch.Tensor.data_ptr()); one launch on ``stream`` (None: the handle's), no
        synchronisation and no allocation."""
        self._check(self.lib.gto_self_clearance_device(self._h, int(B), int(Tp), _vp(paths), float(cutoff), _vp(d2_out),
                                                       _vp(pair_out), _vp(stream)), "gto_self_clearance_device")

    @staticmethod
    def pad_held_points(held_points, n_held=None):
        """(points float64 (B, P_max, 3), counts int32 (B,)) from a list of per-plan (n_i, 3) arrays, or from a padded array
        (B, P_max, 3) with its counts (default: every row counts).  Rows behind a plan's count are zeros and read by nobody."""
        if n_held is None and not (isinstance(held_points, np.ndarray) and held_points.ndim == 3):
            sets = [_f64(p).reshape(-1, 3) for p in held_points]
            counts = _i32([p.shape[0] for p in sets])
            pts = np.zeros((len(sets), max(1, int(counts.max()) if len(sets) else 1), 3))
            for b, p in enumerate(sets):
                pts[b, :p.shape[0]] = p
            return pts, counts
        pts = _f64(held_points)
        if pts.ndim != 3 or pts.shape[2] != 3 or pts.shape[1] < 1:
            raise GTOError(f"held_points: a list of (n_i, 3) arrays or a padded array (B, P_max >= 1, 3); got {pts.shape}")
        counts = _i32(np.broadcast_to(np.asarray(pts.shape[1] if n_held is None else n_held), (pts.shape[0],)))
        return pts, counts

    def _held_inputs(self, who, paths, held_points, n_held, attach, attach_col, object_pose, base_pos):
        """The checked host arrays the held-point entry points share: (paths, points, counts, attach, attach_ld, attach_col,
        pose, base, per_plan_base)."""
        paths = _f64(paths)
        if paths.ndim != 3 or paths.shape[1] != self.desc.ndof or paths.shape[2] < 1:
            raise GTOError(f"{who}: paths must have shape (B, {self.desc.ndof}, Tp >= 1); got {paths.shape}")
        B = paths.shape[0]
        pts, counts = self.pad_held_points(held_points, n_held)
        if pts.shape[0] != B or counts.shape != (B,):
            raise GTOError(f"{who}: one point set and one count per path ({B}); got {pts.shape[0]}, {counts.shape}")
        ld = col = 0
        if attach is not None:
            attach = _f64(attach)
            if attach.ndim != 3 or attach.shape[:2] != (B, self.desc.ndof):
                raise GTOError(f"{who}: attach must have shape ({B}, {self.desc.ndof}, ld); got {attach.shape}")
            ld = attach.shape[2]
            col = ld - 1 if attach_col is None else int(attach_col)
        pose = None if object_pose is None else _f64(object_pose).reshape(B, 16)
        base, per_plan = self._check_base(base_pos, B)
        return paths, pts, counts, attach, ld, col, pose, base, per_plan

    def check_held_paths(self, obs, paths, held_points, n_held=None, attach=None, attach_col=None, object_pose=None, labels=None,
                         held_label=None, base_pos=(0.0, 0.0, 0.0)):
        """gto_check_held_paths: for paths (B, ndof, Tp) the number of plan b's held points inside the observation ``obs`` at
        every column, int32 (B, Tp), the points carried rigidly with link_ee from the configuration the object was grasped
        at: column 0 of the path, or column ``attach_col`` (default: the last) of ``attach`` (B, ndof, ld).  held_points /
        n_held: see ``pad_held_points``; world points at the moment of the grasp, or object-frame points with
        object_pose (B, 4, 4).  labels (H, W) int32 with held_label (B,) or one label: pixels of a depth observation that
        show the held object hide nothing that was seen.  -1: a column, q_att, base or object pose with a non-finite entry."""
        paths, pts, counts, attach, ld, col, pose, base, per_plan = self._held_inputs("check_held_paths", paths, held_points, n_held,
                                                                                      attach, attach_col, object_pose, base_pos)
        B, Tp = paths.shape[0], paths.shape[2]
        lab = None if labels is None else _i32(labels)
        hl = None if held_label is None else _per_instance(held_label, B)
        count = np.empty((B, Tp), dtype=np.int32)
        self._check(self.lib.gto_check_held_paths(self._h, obs._ptr(), B, Tp, _p(paths, _pd), _p(attach, _pd), ld, col, _p(pts, _pd),
                                                  pts.shape[1], _p(counts, _pi), _p(pose, _pd), _p(lab, _pi), _p(hl, _pi),
                                                  _p(base, _pd), per_plan, _p(count, _pi)), "gto_check_held_paths")
        return count

    def check_held_paths_device(self, obs, B, Tp, paths, held_points, P_max, n_held, count_out, attach=None, attach_ld=0,
                                attach_col=0, object_pose=None, labels=None, held_label=None, base_pos=(0.0, 0.0, 0.0),
                                stream=None):
        """gto_check_held_paths_device: paths (B, ndof, Tp), attach, held_points (B, P_max, 3), n_held (B,) int32,
        object_pose (B, 16), labels (H, W) int32, held_label (B,) int32 and count_out (B, Tp) int32 are device pointers (or
        None where the header allows NULL); base_pos is a host value; enqueued on ``stream`` without a host synchronisation."""
        base, per_plan = self._check_base(base_pos, int(B))
        self._check(self.lib.gto_check_held_paths_device(self._h, obs._ptr(), int(B), int(Tp), _vp(paths), _vp(attach), int(attach_ld),
                                                         int(attach_col), _vp(held_points), int(P_max), _vp(n_held),
                                                         _vp(object_pose), _vp(labels), _vp(held_label), _p(base, _pd), per_plan,
                                                         _vp(count_out), _vp(stream)), "gto_check_held_paths_device")

    def held_clearance(self, paths, held_points, n_held=None, attach=None, attach_col=None, object_pose=None,
                       base_pos=(0.0, 0.0, 0.0), links=None, cutoff=np.inf):
        """gto_held_clearance: for paths (B, ndof, Tp) the smallest distance between plan b's held points and the surface
        points of the collision links ``links`` ((L,) bool; None: every link) at every column, the points carried rigidly with
        link_ee as in ``check_held_paths`` (same paths, held_points / n_held, attach / attach_col, object_pose, base_pos).
        Returns a dict: d2 (B, Tp) float64 squared metres, min(d2, cutoff^2); link and point (B, Tp) int32, the closest link
        and held point, -1 where nothing is closer than the cutoff; dist = sqrt(d2).  NaN and -1: a column, q_att, base or
        object pose with a non-finite entry."""
        paths, pts, counts, attach, ld, col, pose, base, per_plan = self._held_inputs("held_clearance", paths, held_points, n_held,
                                                                                      attach, attach_col, object_pose, base_pos)
        B, Tp = paths.shape[0], paths.shape[2]
        mask = held_link_mask(np.ones(self.desc.n_links, dtype=bool) if links is None else links, self.desc.n_links)
        d2, link, point = np.empty((B, Tp)), np.empty((B, Tp), dtype=np.int32), np.empty((B, Tp), dtype=np.int32)
        self._check(self.lib.gto_held_clearance(self._h, B, Tp, _p(paths, _pd), _p(attach, _pd), ld, col, _p(pts, _pd), pts.shape[1],
                                                _p(counts, _pi), _p(pose, _pd), _p(base, _pd), per_plan, mask, float(cutoff),
                                                _p(d2, _pd), _p(link, _pi), _p(point, _pi)), "gto_held_clearance")
        return dict(d2=d2, link=link, point=point, dist=np.sqrt(d2))

    def held_clearance_device(self, B, Tp, paths, held_points, P_max, n_held, d2_out, link_out=None, point_out=None, attach=None,
                              attach_ld=0, attach_col=0, object_pose=None, base_pos=(0.0, 0.0, 0.0), links=None, cutoff=np.inf,
                              stream=None):
        """gto_held_clearance_device: paths (B, ndof, Tp), attach, held_points (B, P_max, 3), n_held (B,) int32, object_pose
        (B, 16), d2_out (B, Tp) float64, link_out and point_out (B, Tp) int32 are device pointers (or None where the header
        allows NULL); base_pos and links ((L,) bool; None: every link) are host values; two launches on ``stream`` without a
        host synchronisation."""
        base, per_plan = self._check_base(base_pos, int(B))
        mask = held_link_mask(np.ones(self.desc.n_links, dtype=bool) if links is None else links, self.desc.n_links)
        self._check(self.lib.gto_held_clearance_device(self._h, int(B), int(Tp), _vp(paths), _vp(attach), int(attach_ld), int(attach_col),
                                                       _vp(held_points), int(P_max), _vp(n_held), _vp(object_pose), _p(base, _pd),
                                                       per_plan, mask, float(cutoff), _vp(d2_out), _vp(link_out), _vp(point_out),
                                                       _vp(stream)), "gto_held_clearance_device")

    # -------------------------------------------------------------- the motion after the grasp
    @staticmethod
    def _closed(closed_joints, closed_values):
        """(indices int32, values float64, count) of the joints a retrieve path holds closed; values may be one scalar."""
        cj = _i32([] if closed_joints is None else closed_joints).reshape(-1)
        cv = _f64(np.broadcast_to(np.asarray(closed_values, dtype=np.float64), cj.shape))
        return cj, cv, int(cj.size)

    def retrieve_lift(self, plans, distance, steps=10, direction=(0.0, 0.0, 1.0), closed_joints=None, closed_values=0.0,
                      scene_id=None, base_pos=None, max_iter=50, pos_tol=0.01, rot_tol_deg=5.0):
        """gto_retrieve_lift: after plans (B, ndof, T), ``steps`` IK steps of link_ee along ``direction`` over ``distance``
        with the gripper's pose held and the joints ``closed_joints`` at ``closed_values``.  Returns a dict of path
        (B, ndof, steps + 1), goals (B, steps, 4, 4), err_pos / err_rot (degrees) / iters / status (B, steps) and reached (B,)."""
        d, T, K = self.desc, self.T, int(steps)
        plans = _f64(plans).reshape(-1, d.ndof, T)
        B = plans.shape[0]
        sid = None if scene_id is None else _per_instance(scene_id, B)
        base = None if base_pos is None else _bases(base_pos, B)
        cj, cv, nc = self._closed(closed_joints, closed_values)
        dirv = _f64(direction).reshape(3)
        Kc = max(K, 0)
        out = dict(path=np.empty((B, d.ndof, Kc + 1)), goals=np.empty((B, Kc, 4, 4)), err_pos=np.empty((B, Kc)),
                   err_rot=np.empty((B, Kc)), iters=np.empty((B, Kc), dtype=np.int32), status=np.empty((B, Kc), dtype=np.int32),
                   reached=np.empty(B, dtype=np.int32))
        self._check(self.lib.gto_retrieve_lift(self._h, B, _p(plans, _pd), _p(sid, _pi), _p(base, _pd), _p(dirv, _pd), float(distance), K,
                                               _p(cj, _pi), _p(cv, _pd), nc, int(max_iter), float(pos_tol), float(rot_tol_deg),
                                               _p(out["path"], _pd), _p(out["goals"], _pd), _p(out["err_pos"], _pd),
                                               _p(out["err_rot"], _pd), _p(out["iters"], _pi), _p(out["status"], _pi),
                                               _p(out["reached"], _pi)), "gto_retrieve_lift")
        return out

    def retrieve_lift_device(self, B, plans, scene_id, base_pos, direction, distance, steps, closed_joints, closed_values, max_iter,
                             pos_tol, rot_tol_deg, path_out, goals_out=None, err_pos_out=None, err_rot_out=None, iters_out=None,
                             status_out=None, reached_out=None, stream=None):
        """gto_retrieve_lift_device: direction, closed_joints and closed_values are HOST values; every other array is a device
        pointer (an int, e.g. torch.Tensor.data_ptr()) or None."""
        cj, cv, nc = self._closed(closed_joints, closed_values)
        dirv = _f64(direction).reshape(3)
        self._check(self.lib.gto_retrieve_lift_device(self._h, int(B), _vp(plans), _vp(scene_id), _vp(base_pos), _p(dirv, _pd),
                                                      float(distance), int(steps), _p(cj, _pi), _p(cv, _pd), nc, int(max_iter),
                                                      float(pos_tol), float(rot_tol_deg), _vp(path_out), _vp(goals_out),
                                                      _vp(err_pos_out), _vp(err_rot_out), _vp(iters_out), _vp(status_out),
                                                      _vp(reached_out), _vp(stream)), "gto_retrieve_lift_device")

    def retrieve_path_columns(self):
        """gto_retrieve_path_columns: columns of the reversed path (19 at the defaults); -1 when the horizon is too short."""
        return int(self.lib.gto_retrieve_path_columns(self._h))

    def retrieve_reverse(self, B, plans, closed_joints, closed_values, path_out, stream=None):
        """gto_retrieve_reverse_device: plans (B, ndof, T) and path_out (B, ndof, n) are device pointers; returns n."""
        cj, cv, nc = self._closed(closed_joints, closed_values)
        n = C.c_int32(0)
        self._check(self.lib.gto_retrieve_reverse_device(self._h, int(B), _vp(plans), _p(cj, _pi), _p(cv, _pd), nc, _vp(path_out),
                                                         C.byref(n), _vp(stream)), "gto_retrieve_reverse_device")
        return int(n.value)

    # -------------------------------------------------------------- retiming
    def _retime_limits(self, vmax, amax):
        nd = self.desc.ndof
        return (_f64(np.broadcast_to(np.asarray(vmax, dtype=np.float64), (nd,))),
                _f64(np.broadcast_to(np.asarray(amax, dtype=np.float64), (nd,))))

    def retime_batch(self, plans, vmax, amax, subdiv: int = 2, n_samples: int = 100):
        """gto_retime_batch: time-optimal retiming of plans (B, ndof, T) under joint velocity limits vmax and acceleration
        limits amax (each (ndof,) or a scalar; vmax may hold +inf).  Returns a dict of duration (B,), t_grid (B, N),
        sd_grid (B, N), q / qd / qdd (B, n_samples, ndof) and status (B,), N = subdiv (T-1) + 1."""
        d, T = self.desc, self.T
        plans = _f64(plans).reshape(-1, d.ndof, T)
        B, N, M = plans.shape[0], int(subdiv) * (T - 1) + 1, int(n_samples)
        vm, am = self._retime_limits(vmax, amax)
        out = dict(duration=np.empty(B), t_grid=np.empty((B, max(N, 0))), sd_grid=np.empty((B, max(N, 0))),
                   q=np.empty((B, max(M, 0), d.ndof)), qd=np.empty((B, max(M, 0), d.ndof)), qdd=np.empty((B, max(M, 0), d.ndof)),
                   status=np.empty(B, dtype=np.int32))
        self._check(self.lib.gto_retime_batch(self._h, B, _p(plans, _pd), _p(vm, _pd), _p(am, _pd), int(subdiv), M,
                                              _p(out["duration"], _pd), _p(out["t_grid"], _pd), _p(out["sd_grid"], _pd),
                                              _p(out["q"], _pd), _p(out["qd"], _pd), _p(out["qdd"], _pd),
                                              _p(out["status"], _pi)), "gto_retime_batch")
        return out

    def retime_batch_device(self, B, plans, vmax, amax, subdiv, n_samples, duration_out=None, t_grid_out=None,
                            sd_grid_out=None, q_out=None, qd_out=None, qdd_out=None, status_out=None, stream=None):
        """gto_retime_batch_device: plans and outputs are device pointers (ints, e.g. torch.Tensor.data_ptr()) or None;
        vmax / amax are host values."""
        vm, am = self._retime_limits(vmax, amax)
        self._check(self.lib.gto_retime_batch_device(self._h, int(B), _vp(plans), _p(vm, _pd), _p(am, _pd), int(subdiv),
                                                     int(n_samples), _vp(duration_out), _vp(t_grid_out), _vp(sd_grid_out),
                                                     _vp(q_out), _vp(qd_out), _vp(qdd_out), _vp(status_out), _vp(stream)),
                    "gto_retime_batch_device")

    def retime_paths(self, paths, vmax, amax, n_cols=None, subdiv: int = 2, n_samples: int = 100):
        """gto_retime_paths: retime_batch for paths (B, ndof, Tp) of any length Tp >= 2, on any handle.  n_cols (B,) int:
        path b is its first n_cols[b] columns (None: all Tp); the rest is ignored.  Returns the dict of retime_batch with
        t_grid / sd_grid (B, Nmax), Nmax = subdiv (Tp-1) + 1: past a path's own subdiv (n_cols[b]-1) + 1 gridpoints they hold
        the duration and 0.  A count outside [1, Tp] raises."""
        d = self.desc
        paths = _f64(paths)
        if paths.ndim != 3 or paths.shape[1] != d.ndof:
            raise ValueError(f"retime_paths: paths must be (B, {d.ndof}, Tp), got {paths.shape}")
        B, Tp, M = paths.shape[0], paths.shape[2], int(n_samples)
        N = max(int(subdiv) * (Tp - 1) + 1, 0)
        nc = None if n_cols is None else _per_instance(n_cols, B)
        vm, am = self._retime_limits(vmax, amax)
        out = dict(duration=np.empty(B), t_grid=np.empty((B, N)), sd_grid=np.empty((B, N)),
                   q=np.empty((B, max(M, 0), d.ndof)), qd=np.empty((B, max(M, 0), d.ndof)), qdd=np.empty((B, max(M, 0), d.ndof)),
                   status=np.empty(B, dtype=np.int32))
        self._check(self.lib.gto_retime_paths(self._h, B, Tp, _p(paths, _pd), _p(nc, _pi), _p(vm, _pd), _p(am, _pd), int(subdiv), M,
                                              _p(out["duration"], _pd), _p(out["t_grid"], _pd), _p(out["sd_grid"], _pd),
                                              _p(out["q"], _pd), _p(out["qd"], _pd), _p(out["qdd"], _pd),
                                              _p(out["status"], _pi)), "gto_retime_paths")
        return out

    def retime_paths_convex(self, paths, vmax, amax, n_cols=None, subdiv: int = 2, n_samples: int = 100,
                            gap_tol: float = 1e-8, max_newton: int = RETIME_MAX_NEWTON):
        """gto_retime_paths_convex: retime_paths with the grid's time-optimal profile (a convex program per path, solved to
        a certified relative gap gap_tol in at most max_newton Newton steps) in place of the greedy one.  Returns the dict
        of retime_paths and iters (B,), the Newton steps taken; status 1 (GTO_STATUS_MAX_ITER): a feasible profile with valid
        samples whose gap is not certified."""
        d = self.desc
        paths = _f64(paths)
        if paths.ndim != 3 or paths.shape[1] != d.ndof:
            raise ValueError(f"retime_paths_convex: paths must be (B, {d.ndof}, Tp), got {paths.shape}")
        B, Tp, M = paths.shape[0], paths.shape[2], int(n_samples)
        N = max(int(subdiv) * (Tp - 1) + 1, 0)
        nc = None if n_cols is None else _per_instance(n_cols, B)
        vm, am = self._retime_limits(vmax, amax)
        out = dict(duration=np.empty(B), t_grid=np.empty((B, N)), sd_grid=np.empty((B, N)),
                   q=np.empty((B, max(M, 0), d.ndof)), qd=np.empty((B, max(M, 0), d.ndof)), qdd=np.empty((B, max(M, 0), d.ndof)),
                   status=np.empty(B, dtype=np.int32), iters=np.empty(B, dtype=np.int32))
        self._check(self.lib.gto_retime_paths_convex(self._h, B, Tp, _p(paths, _pd), _p(nc, _pi), _p(vm, _pd), _p(am, _pd),
                                                     int(subdiv), M, float(gap_tol), int(max_newton),
                                                     _p(out["duration"], _pd), _p(out["t_grid"], _pd), _p(out["sd_grid"], _pd),
                                                     _p(out["q"], _pd), _p(out["qd"], _pd), _p(out["qdd"], _pd),
                                                     _p(out["status"], _pi), _p(out["iters"], _pi)), "gto_retime_paths_convex")
        return out

    def retime_paths_torque(self, paths, vmax, amax, tau_max=None, payload=None, n_cols=None, subdiv: int = 2,
                            n_samples: int = 100, gap_tol: float = 1e-8, max_newton: int = RETIME_MAX_NEWTON):
        """gto_retime_paths_torque: retime_paths_convex with joint torque limits ``tau_max`` ((ndof,) or one value, +inf = no
        limit; None = the description's effort limits) on top of vmax / amax, the held object included: ``payload`` is the
        dict of ``inverse_dynamics`` ("mass" and optionally "com", "inertia" on the end-effector frame), each entry one
        value for the call or one per path.  Returns the dict of retime_paths_convex and tau (B, n_samples, ndof), the joint
        forces at the samples; status 3 (GTO_STATUS_INFEASIBLE): some joint cannot hold the path at rest, NaN outputs."""
        d = self.desc
        paths = _f64(paths)
        if paths.ndim != 3 or paths.shape[1] != d.ndof:
            raise ValueError(f"retime_paths_torque: paths must be (B, {d.ndof}, Tp), got {paths.shape}")
        B, Tp, M = paths.shape[0], paths.shape[2], int(n_samples)
        N = max(int(subdiv) * (Tp - 1) + 1, 0)
        nc = None if n_cols is None else _per_instance(n_cols, B)
        vm, am = self._retime_limits(vmax, amax)
        tm = retime_torque_limits(d, tau_max, need_inertials=False)
        pm, pc, pi = payload_arrays(payload, B)
        self.sync_link_inertials()
        out = dict(duration=np.empty(B), t_grid=np.empty((B, N)), sd_grid=np.empty((B, N)),
                   q=np.empty((B, max(M, 0), d.ndof)), qd=np.empty((B, max(M, 0), d.ndof)), qdd=np.empty((B, max(M, 0), d.ndof)),
                   tau=np.empty((B, max(M, 0), d.ndof)), status=np.empty(B, dtype=np.int32), iters=np.empty(B, dtype=np.int32))
        self._check(self.lib.gto_retime_paths_torque(self._h, B, Tp, _p(paths, _pd), _p(nc, _pi), _p(vm, _pd), _p(am, _pd),
                                                     _p(tm, _pd), _p(pm, _pd), _p(pc, _pd), _p(pi, _pd), int(subdiv), M,
                                                     float(gap_tol), int(max_newton), _p(out["duration"], _pd),
                                                     _p(out["t_grid"], _pd), _p(out["sd_grid"], _pd), _p(out["q"], _pd),
                                                     _p(out["qd"], _pd), _p(out["qdd"], _pd), _p(out["tau"], _pd),
                                                     _p(out["status"], _pi), _p(out["iters"], _pi)), "gto_retime_paths_torque")
        return out

    def retime_paths_torque_device(self, B, Tp, paths, vmax, amax, tau_max=None, payload_mass=None, payload_com=None,
                                   payload_inertia=None, n_cols=None, subdiv=2, n_samples=100, gap_tol=1e-8,
                                   max_newton=RETIME_MAX_NEWTON, duration_out=None, t_grid_out=None, sd_grid_out=None,
                                   q_out=None, qd_out=None, qdd_out=None, tau_out=None, status_out=None, iters_out=None,
                                   stream=None):
        """gto_retime_paths_torque_device: retime_paths_convex_device with torque limits (host values; None = the
        description's effort limits); payload_mass (B,), payload_com (B, 3), payload_inertia (B, 6) and tau_out
        (B, n_samples, ndof) are device pointers or None."""
        vm, am = self._retime_limits(vmax, amax)
        tm = retime_torque_limits(self.desc, tau_max, need_inertials=False)
        self.sync_link_inertials()
        self._check(self.lib.gto_retime_paths_torque_device(self._h, int(B), int(Tp), _vp(paths), _vp(n_cols), _p(vm, _pd),
                                                            _p(am, _pd), _p(tm, _pd), _vp(payload_mass), _vp(payload_com),
                                                            _vp(payload_inertia), int(subdiv), int(n_samples), float(gap_tol),
                                                            int(max_newton), _vp(duration_out), _vp(t_grid_out),
                                                            _vp(sd_grid_out), _vp(q_out), _vp(qd_out), _vp(qdd_out),
                                                            _vp(tau_out), _vp(status_out), _vp(iters_out), _vp(stream)),
                    "gto_retime_paths_torque_device")

    def retime_paths_convex_device(self, B, Tp, paths, vmax, amax, n_cols=None, subdiv=2, n_samples=100, gap_tol=1e-8,
                                   max_newton=RETIME_MAX_NEWTON, duration_out=None, t_grid_out=None, sd_grid_out=None,
                                   q_out=None, qd_out=None, qdd_out=None, status_out=None, iters_out=None, stream=None):
        """gto_retime_paths_convex_device: retime_paths_device with the convex profile; iters_out (B,) int32 is a device
        pointer or None."""
        vm, am = self._retime_limits(vmax, amax)
        self._check(self.lib.gto_retime_paths_convex_device(self._h, int(B), int(Tp), _vp(paths), _vp(n_cols), _p(vm, _pd),
                                                            _p(am, _pd), int(subdiv), int(n_samples), float(gap_tol),
                                                            int(max_newton), _vp(duration_out), _vp(t_grid_out),
                                                            _vp(sd_grid_out), _vp(q_out), _vp(qd_out), _vp(qdd_out),
                                                            _vp(status_out), _vp(iters_out), _vp(stream)),
                    "gto_retime_paths_convex_device")

    def retime_paths_device(self, B, Tp, paths, vmax, amax, n_cols=None, subdiv=2, n_samples=100, duration_out=None,
                            t_grid_out=None, sd_grid_out=None, q_out=None, qd_out=None, qdd_out=None, status_out=None,
                            stream=None):
        """gto_retime_paths_device: paths (B, ndof, Tp), n_cols (B,) int32 and the outputs are device pointers (ints, e.g.
        torch.Tensor.data_ptr()) or None; vmax / amax are host values.  A count outside [1, Tp] is not seen by the host:
        that path gets GTO_STATUS_NUMERICAL and NaN."""
        vm, am = self._retime_limits(vmax, amax)
        self._check(self.lib.gto_retime_paths_device(self._h, int(B), int(Tp), _vp(paths), _vp(n_cols), _p(vm, _pd), _p(am, _pd),
                                                     int(subdiv), int(n_samples), _vp(duration_out), _vp(t_grid_out),
                                                     _vp(sd_grid_out), _vp(q_out), _vp(qd_out), _vp(qdd_out), _vp(status_out),
                                                     _vp(stream)), "gto_retime_paths_device")
