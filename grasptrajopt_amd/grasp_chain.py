"""GraspChain — the per-object loop of the reference's driver after perception (examples/pybullet_gto_planning.py:192-294)
on one stream:

    object poses and object-frame grasps -> the grasp collision filter against each object's observation, the base-frame
    goal sets compacted (gto_filter_grasps_device; ``plan_grasps``, :192-236) ->
    grasp poses (``plan_objects`` starts here, :242) -> IK (gto_solve_ik_pose_batch_device) -> err_pos / err_rot /
    collision cost and the acceptance test of :262 (gto_ik_report_device) -> accepted goal sets and seeds (gto_seed_goalsets_device) -> gto_solve_batch_device ->
    optionally gto_check_plans_device, the retrieve motion after the grasp (:301-313: gto_retrieve_lift_device or
    gto_retrieve_reverse_device, with gto_check_paths_device and, for the object the robot holds,
    gto_check_held_paths_device), gto_retime_batch_device and, for the retrieve path, gto_retime_paths_device

(with ``n_seeds`` > 1: gto_seed_goalsets_multi_device -> one gto_solve_batch_device over every object's n_seeds best seeds ->
gto_plan_report_device -> gto_check_plans_device -> gto_select_plans_device, and the best plan of every object goes on)

for many objects at once, with ONE host synchronisation at the end.  ``IKSolver.solve_ik_batch`` + the filter on the host +
``GTOPlanner.plan_goalset`` compute the same thing object by object with a host round trip between the steps; the plans
are bit-equal (the same seed and goals go into the same solve).
"""
from __future__ import annotations

import inspect
from types import SimpleNamespace

import numpy as np

from . import _capi
from .synthetic import standoff_pose


def finger_joints(desc):
    """The robot's parameter joints that are fingers (the configs' finger_index): what the driver closes after the grasp."""
    return [int(i) for i in desc.param_index if "finger" in desc.actuated_joint_names[int(i)]]


class GraspChain:
    def __init__(self, robot, link_ee, link_gripper, standoff_distance=-0.1, standoff_offset=-10, device=0):
        import torch
        self.robot, self.link_ee, self.link_gripper = robot, link_ee, link_gripper
        self.standoff_distance, self.standoff_offset = standoff_distance, standoff_offset
        self.T = 50            # gto/gto_planner.py:25
        self.Tmax = 10.0       # :26
        self.max_iter = 100    # :141
        self.ik_max_iter = 50  # gto/ik_solver.py:76
        opts = _capi.default_opts()
        dt = self.Tmax / (self.T - 1)
        opts.T, opts.Tmax, opts.standoff_offset = self.T, dt * (self.T - 1), standoff_offset  # (GTOPlanner's horizon, bit for bit)
        opts.w_obstacle, opts.w_vel, opts.max_iter = 10.0, 0.01, self.max_iter  # :114,:130 and gto/ik_solver.py:70
        self._handle = _capi.SolverHandle(robot.desc, link_ee, link_gripper, opts, device=device)
        self._torch = torch
        self.device = torch.device("cuda", device)
        self.stream = torch.cuda.Stream(device=self.device)
        self._handle.set_stream(self.stream.cuda_stream)
        self._buf = {}

    def close(self):
        if self._handle is not None:
            self._torch.cuda.synchronize(self.device)
            self._handle.close()
            self._handle = None
            self._buf = {}

    # ------------------------------------------------------------------ scenes
    def bind_scene(self, sid, sdf_cost_all, sdf_cost_obstacle):
        """Scene ``sid`` of the chain's handle from a pair of cost fields: two fields of one resident scene
        (depth_scene.LazyCostField) are shared in as ``IKSolver._bind_scene`` shares them, arrays are uploaded.  A scene
        that is bound stays: ``plan_objects`` takes its id in place of a pair of fields."""
        from .depth_scene import resident_of
        h = self._handle
        ro, ra = resident_of(sdf_cost_obstacle), resident_of(sdf_cost_all)  # the obstacle field first: its build holds both fields
        if ro is not None and ra is not None and ra.handle is ro.handle and (ra.sid, ra.gen) == (ro.sid, ro.gen):
            # (shared again on every call: a later build of the resident scene leaves no stale pointer behind)
            h.share_scene(sid, ro.handle, ro.sid, all_from=ra.half, obs_from=ro.half)
        else:
            shape, origin, res = self.robot.field_geometry()
            h.set_scene(sid, np.asarray(sdf_cost_all), np.asarray(sdf_cost_obstacle), shape, origin, res)
        return sid

    def _scene_ids(self, fields, B):
        """Scene id of every object: ``fields`` is one entry for all objects or one per object; an entry is the id of a bound
        scene or a pair (sdf_cost_all, sdf_cost_obstacle); objects that name the same pair share one scene."""
        one = isinstance(fields, (int, np.integer)) or (isinstance(fields, tuple) and len(fields) == 2 and not isinstance(fields[0], tuple))
        entries = [fields] * B if one else list(fields)
        if len(entries) != B:
            raise ValueError(f"fields: one entry for all objects or one per object ({B}), got {len(entries)}")
        taken = {int(e) for e in entries if isinstance(e, (int, np.integer))}
        ids, seen, nxt = [], {}, 0
        for e in entries:
            if isinstance(e, (int, np.integer)):
                ids.append(int(e))
                continue
            key = (id(e[0]), id(e[1]))
            if key not in seen:
                while nxt in taken:
                    nxt += 1
                seen[key] = self.bind_scene(nxt, e[0], e[1])
                taken.add(nxt)
            ids.append(seen[key])
        return np.asarray(ids, dtype=np.int32)

    # ------------------------------------------------------------------ buffers
    def _dev(self, name, shape, dtype):
        """A device buffer of the chain, kept between calls while the shape stays."""
        t = self._buf.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = self._torch.empty(tuple(shape), dtype=dtype, device=self.device)
            self._buf[name] = t
        return t

    def _pin(self, name, shape, dtype):
        """A pinned host buffer of the chain (a call ends with a synchronisation: nothing is in flight when it is reused)."""
        t = self._buf.get("pin/" + name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = self._torch.empty(tuple(shape), dtype=dtype, pin_memory=True)
            self._buf["pin/" + name] = t
        return t

    def _up(self, name, array, dtype):
        """Host array -> the chain's device buffer of that name, through pinned memory, enqueued on the current stream."""
        src = self._torch.from_numpy(np.require(array, dtype=dtype, requirements=["C", "W"]))  # (a read-only view is copied)
        pin = self._pin(name, src.shape, src.dtype)
        pin.copy_(src)
        dst = self._dev(name, src.shape, src.dtype)
        dst.copy_(pin, non_blocking=True)
        return dst

    # ------------------------------------------------------------------ the chain
    def plan_objects(self, qc, ik_goals, plan_goals, n_grasps, fields, base_position, axis_standoff="x", use_standoff=True,
                     interpolate=True, pos_tol=0.01, rot_tol_deg=5.0, ik_collision_threshold=5.0, float32_solutions=True,
                     observation=None, retime=None, n_seeds=1, max_points=5, retrieve=None, track=None, self_check=None):
        """B objects with up to n_max candidate grasps each.

        qc (B, ndof) or (ndof,); ik_goals, plan_goals (B, n_max, 4, 4): the poses IK is solved to and the poses the plan
        goes to (the shelf driver solves IK to ``RT @ standoff`` and plans to ``RT``, :256-259); n_grasps (B,) how many rows
        of an object count; fields: see ``_scene_ids``; base_position (3,) or (B, 3).  observation: an
        ``observation.Observation`` to count the solved plans' surface points inside (gto_check_plans_device).  retime: a
        dict ``vmax, amax[, subdiv, n_samples, profile, gap_tol, max_newton, tau_max, payload]`` to retime the solved plans
        (gto_retime_batch_device; ``profile="convex"``: the grid's time optimum, gto_retime_paths_convex_device for the plans
        and the retrieve path alike, which adds retime_iters / retrieve_retime_iters (B,); ``profile="torque"``: that optimum
        under the joint torque limits ``tau_max`` too (None: the description's effort limits), gto_retime_paths_torque_device
        -- the approach plans with an empty hand, the retrieve path with ``payload``, the dict of
        ``SolverHandle.inverse_dynamics`` with one value per call or per object; with ``retrieve_samples`` the result also
        has retrieve_tau (B, n_samples, ndof)).  retrieve: a dict
        ``mode`` ("lift" | "reverse") ``[, distance, steps, direction, closed_joints, closed_value, collide]`` for the motion
        after the grasp (see ``retrieve_spec``), enqueued behind the solve (with n_seeds > 1 behind the selection) on the
        chain's stream; the result gains retrieve_path (B, ndof, steps + 1 | n), retrieve_reached (B,) (lift: the leading
        steps that reached their goal; reverse: n), retrieve_status (B, steps) (reverse: (B, 0)) and, with an observation,
        retrieve_counts (B, columns); with an observation and ``held_points`` in the retrieve dict also
        retrieve_held_counts (B, columns): how many points of the object the robot holds are inside the observation at every
        column (gto_check_held_paths_device, enqueued behind the robot's own check); with ``held_points`` and ``held_clearance``
        in the retrieve dict (no observation needed) also retrieve_held_self_d2, retrieve_held_self_col,
        retrieve_held_self_link, retrieve_held_self_point and retrieve_held_self_clear (B,): the held points' smallest
        squared distance from the robot's own links over the path's columns, where, and whether every column keeps the
        clearance (gto_held_clearance_device, one call on the chain's stream in front of the one synchronisation;
        ``_capi.held_clearance_summary``).  With retrieve AND retime the retrieve path is retimed too, under the same limits,
        subdiv and n_samples, on the chain's stream behind the retrieve stage (gto_retime_paths_device; ``reached_only`` in
        the retrieve dict: only columns 0 .. reached of a lift, the count made from retrieve_reached on the stream): the
        result gains retrieve_durations, retrieve_retime_status (B,) and, with ``retrieve_samples`` set in the retime dict,
        retrieve_q / retrieve_qd / retrieve_qdd (B, n_samples, ndof).  track: a dict ``kp, kd[, tau_max, dt, settle,
        feedforward, model_payload, plant_payload, locked]`` (the keywords of ``utils.track_trajectories``) to roll the
        retimed trajectories forward under that joint controller (gto_track_rollout_device), on the chain's stream behind the
        retime calls with no further synchronisation; it needs ``retime``.  The approach is rolled out with an empty hand;
        the retrieve path with each object's payload in the hand -- ``plant_payload``, default the retime dict's ``payload``
        -- which the controller knows unless ``model_payload`` says otherwise.  The result gains track_err_max,
        track_err_end, track_sat_steps, track_status (B,) and, with retrieve, the four retrieve_track_*.  The chain keeps the
        samples the rollout reads in its own device buffers.  track=None leaves the chain launch for launch what it is.
        self_check: a dict ``[clearance, cutoff, mask, q_ref]`` (``_capi.self_check_request``; {} for the defaults) to
        measure the robot's clearance from ITSELF along the selected plan and, with retrieve, along the retrieve path
        (gto_self_clearance_device, one launch each on the chain's stream in front of the one synchronisation).  The result
        gains self_d2 (B,) (the smallest squared distance over the plan's waypoints, metres^2, at most cutoff^2; NaN for a
        plan with a non-finite waypoint), self_pair (B, 2) (the closest link pair there, (-1, -1) when far), self_clear (B,)
        (every waypoint at least ``clearance`` away) and their retrieve_self_* counterparts.  plan_class and the selection
        do not read them.  Like the retime and retrieve results, the keys are absent when the call holds no candidate grasp
        at all (B * n_max = 0): nothing was solved, so nothing is checked.  self_check=None leaves the chain launch for
        launch what it is.

        Returns a namespace: plans (B, ndof, T), dQ (B, ndof, T-1), cost, iters, status (B,), n_accepted (B,) (0: no
        feasible grasp, the driver's ``continue``; the plan is then the solve from the constant seed to all goals),
        seed_index (B,) (position among the accepted, -1 without one), seed_cost, seed_dist (B, n_max), q_solutions
        (B, n_max, ndof) (float32 with float32_solutions), err_pos, err_rot, ik_cost, ik_iters, ik_status, accept
        (B, n_max), and counts (B, T) / durations, retime_status (B,) when asked for.

        n_seeds > 1 solves every object from its n_seeds best seeds (np.lexsort((dist, cost))[:n_seeds]) in one solve of
        B * n_seeds instances and keeps the best plan: the lowest class (0 reached within pos_tol / rot_tol_deg and no
        waypoint with more than max_points surface points inside the observation, 1 free, 2 reached, 3 neither, 4 a solve
        that ended numerically), then the lowest cost, then the lowest slot.  plans, dQ, cost, iters, status, counts are the
        chosen slot's; seed_index becomes (B, n_seeds) (-1: a slot behind the accepted grasps, which solves slot 0 again);
        added: best_slot, plan_class (B,), goal_index (B,) (the compacted position of the grasp the plan reached), goal_row
        (B,) (its row among the object's grasps: where to close the gripper; -1 without an accepted grasp), plan_err_pos,
        plan_err_rot (B,), slot_cost, slot_class (B, n_seeds), slot_plans (B, n_seeds, ndof, T).  n_seeds = 1 is the chain above, launch for launch."""
        ik_goals = np.asarray(ik_goals, dtype=np.float64)
        B, n_max = ik_goals.shape[0], ik_goals.shape[1]
        ik_goals = ik_goals.reshape(B, n_max, 16)
        plan_goals = np.asarray(plan_goals, dtype=np.float64).reshape(B, n_max, 16)
        n_grasps = self._grasp_counts(n_grasps, B, n_max)

        def feed(st, d_base):
            return (self._up("ik_goals", ik_goals, np.float64), self._up("plan_goals", plan_goals, np.float64),
                    self._up("n_grasps", n_grasps, np.int32), {})

        return self._plan(B, n_max, feed, qc, fields, base_position, axis_standoff, use_standoff, interpolate, pos_tol, rot_tol_deg,
                          ik_collision_threshold, float32_solutions, observation, retime, n_seeds, max_points, retrieve, track,
                          self_check)

    def retrieve_spec(self, retrieve):
        """A ``retrieve`` dict with its defaults filled in: mode "lift" (straight up by ``distance`` = 0.3 m in ``steps`` = 10
        IK steps along ``direction`` = (0, 0, 1) with the gripper's pose held; ``collide``: with the collision term of the
        object's scene, default False as in the reference's retract) or "reverse" (the plan's last stretch backwards);
        ``closed_joints`` (default: the robot's parameter joints that are fingers) are held at ``closed_value`` = 0;
        ``reached_only`` (lift, with a ``retime`` dict): retime columns 0 .. reached of the path, not all of it.
        ``held_points`` (with an observation): the points of the object every plan holds, a list of B (n_i, 3) arrays or a
        padded array (B, P_max, 3) with ``held_counts`` (B,); world points at the moment of the grasp, or object-frame points
        with ``object_pose`` (B, 4, 4) (``plan_grasps`` places object-frame points at its own object poses when the key is
        absent); ``labels`` (H, W) int32 and ``held_label`` (B,) or one label: the segmentation image of a depth observation
        and the held object's label in it, whose pixels hide nothing that was seen (include/gto_solver.h).
        ``held_clearance`` (with ``held_points``; no observation needed): a dict ``[clearance, cutoff, links, ignore]``
        (``_capi.held_clearance_request``; {} for the defaults) to measure the held points' clearance from the robot's own
        links along the retrieve path (gto_held_clearance_device)."""
        known = {"mode", "distance", "steps", "direction", "closed_joints", "closed_value", "collide", "reached_only", "held_points",
                 "held_counts", "object_pose", "labels", "held_label", "held_clearance"}
        if set(retrieve) - known:
            raise TypeError(f"retrieve: unexpected key(s) {sorted(set(retrieve) - known)}")
        r = dict(mode="lift", distance=0.3, steps=10, direction=(0.0, 0.0, 1.0), closed_joints=None, closed_value=0.0, collide=False,
                 reached_only=False, held_points=None, held_counts=None, object_pose=None, labels=None, held_label=None,
                 held_clearance=None)
        r.update(retrieve)
        if r["mode"] not in ("lift", "reverse"):
            raise ValueError('retrieve: mode is "lift" or "reverse"')
        if r["closed_joints"] is None:
            r["closed_joints"] = finger_joints(self.robot.desc)
        return r

    def plan_grasps(self, qc, object_poses, grasps, n_grasps, observations, fields, base_position, gripper_points, check_offset,
                    ik_offset=None, world_to_base=None, max_ratio=0.01, **plan_objects_keywords):
        """The driver's whole per-object loop after perception (:192-294): the grasp collision filter, then ``plan_objects``,
        with the one synchronisation at the end.

        object_poses (B, 4, 4); grasps (B, n_max, 4, 4) in the object's frame; n_grasps (B,); observations: one entry for all
        objects or one per object, an ``observation.Observation`` or a DepthPointCloud / SurfacePointCloud (its cached
        observation); gripper_points (P, 3): the open gripper's surface points in the frame the poses place; check_offset
        (4, 4): the pose the points are placed at relative to the grasp (the driver's get_standoff_pose(offset, axis));
        ik_offset (4, 4) or None: the shelf driver solves IK to ``RT @ standoff`` (:256-259); world_to_base (B, 4, 4) or None:
        the mobile driver's inv(RT_base); a grasp is kept when count / P <= max_ratio.  base_position is subtracted from the
        goals (:254) and serves the chain as in ``plan_objects``, whose other keywords pass through.

        gto_filter_grasps_device writes the goal sets ``plan_objects`` would be given (``utils.filter_grasp_sets`` computes
        them on the host), and exactly its launches follow.  Added to its result: grasp_counts (B, n_max) (-1: a non-finite
        row; rows beyond n_grasps are -1 too), grasp_keep (B, n_max), kept_rows (B, n_max) (the original row of a compacted
        position, -1 beyond the kept ones), n_kept (B,) (0: no collision-free grasp, the driver's ``continue`` at :236; the
        object is then solved to its row 0), grasp_row (B,): the ORIGINAL row of the grasp the plan was seeded from -- with
        n_seeds > 1 of the grasp it reached --, -1 without a kept or an accepted grasp.  accept, q_solutions, err_pos and the
        other per-candidate arrays are indexed by compacted position."""
        from .observation import as_observation
        torch = self._torch
        object_poses = np.asarray(object_poses, dtype=np.float64).reshape(-1, 16)
        B = object_poses.shape[0]
        grasps = np.asarray(grasps, dtype=np.float64)
        n_max = grasps.shape[1]
        grasps = grasps.reshape(B, n_max, 16)
        n_grasps = self._grasp_counts(n_grasps, B, n_max)
        points = np.asarray(gripper_points, dtype=np.float64).reshape(-1, 3)
        one = not isinstance(observations, (list, tuple))
        obs = [as_observation(o) for o in ([observations] * B if one else observations)]
        if len(obs) != B:
            raise ValueError(f"observations: one entry for all objects or one per object ({B}), got {len(obs)}")
        w2b = None if world_to_base is None else np.asarray(world_to_base, dtype=np.float64).reshape(B, 16)
        f64, i32, u8 = torch.float64, torch.int32, torch.uint8

        def feed(st, d_base):
            d_op, d_gr = self._up("object_poses", object_poses, np.float64), self._up("grasps", grasps, np.float64)
            d_n, d_pts = self._up("n_grasps_in", n_grasps, np.int32), self._up("gripper_points", points, np.float64)
            d_w = None if w2b is None else self._up("world_to_base", w2b, np.float64)
            d_ikg, d_pg = self._dev("ik_goals", (B, n_max, 16), f64), self._dev("plan_goals", (B, n_max, 16), f64)
            d_ng, d_nk = self._dev("n_grasps", (B,), i32), self._dev("n_kept", (B,), i32)
            d_fc, d_keep = self._dev("grasp_counts", (B, n_max), i32), self._dev("grasp_keep", (B, n_max), u8)
            d_rows = self._dev("kept_rows", (B, n_max), i32)
            d_ikg.zero_()  # positions behind an object's kept grasps are solved by IK and read by nobody: defined all the same
            d_pg.zero_()
            d_keep.zero_()
            d_fc.fill_(-1)
            d_rows.fill_(-1)
            if B:
                self._handle.filter_grasps_device(obs, n_max, d_pts.data_ptr(), points.shape[0], d_op.data_ptr(), d_gr.data_ptr(),
                                                  d_n.data_ptr(), check_offset, ik_offset, None if d_w is None else d_w.data_ptr(),
                                                  d_base.data_ptr(), max_ratio, d_fc.data_ptr(), d_keep.data_ptr(), d_rows.data_ptr(),
                                                  d_nk.data_ptr(), d_ng.data_ptr(), d_pg.data_ptr(), d_ikg.data_ptr(), st)
            return d_ikg, d_pg, d_ng, dict(grasp_counts=d_fc, grasp_keep=d_keep, kept_rows=d_rows, n_kept=d_nk, _object_pose=d_op)

        kw = {k: p.default for k, p in inspect.signature(self.plan_objects).parameters.items() if p.default is not p.empty}
        unknown = set(plan_objects_keywords) - set(kw)
        if unknown:
            raise TypeError(f"plan_grasps: unexpected keyword(s) {sorted(unknown)}")
        kw.update(plan_objects_keywords)
        res = self._plan(B, n_max, feed, qc, fields, base_position, **kw)
        res.grasp_keep = res.grasp_keep.astype(bool)
        rows = np.arange(B)
        if int(kw["n_seeds"]) != 1:
            pos = res.goal_row  # the compacted position of the grasp the plan reached
        else:  # the seed's position among the accepted -> its compacted position
            counted = res.accept & (np.arange(n_max)[None, :] < np.maximum(res.n_kept, 1)[:, None])
            order = np.argsort(~counted, axis=1, kind="stable")  # the accepted positions first, in their order
            pos = np.where(res.seed_index >= 0, order[rows, np.maximum(res.seed_index, 0)], -1)
        known = (res.n_kept > 0) & (res.n_accepted > 0) & (pos >= 0)
        res.grasp_row = np.where(known, res.kept_rows[rows, np.maximum(pos, 0)], -1).astype(np.int32)
        return res

    @staticmethod
    def _grasp_counts(n_grasps, B, n_max):
        n_grasps = np.ascontiguousarray(np.broadcast_to(np.asarray(n_grasps, dtype=np.int32), (B,)))
        if B and (n_grasps.min() < 1 or n_grasps.max() > n_max):
            raise ValueError("n_grasps must be in [1, n_max]")
        return n_grasps

    def _plan(self, B, n_max, feed, qc, fields, base_position, axis_standoff, use_standoff, interpolate, pos_tol, rot_tol_deg,
              ik_collision_threshold, float32_solutions, observation, retime, n_seeds, max_points, retrieve=None, track=None,
              self_check=None):
        """What ``plan_objects`` and ``plan_grasps`` share: the chain from the goal sets on.  ``feed(stream, d_base)`` is called
        on the chain's stream behind the uploads of scene ids, qc and base; it returns the device arrays ik_goals, plan_goals
        (B, n_max, 16), n_grasps (B,) -- uploaded, or written by launches it enqueued -- and a dict of further device arrays
        to bring back with the result."""
        K = int(n_seeds)
        multi = K != 1  # K slots per object, a slot being one instance of the solve
        torch, h, d = self._torch, self._handle, self.robot.desc
        ndof, T = d.ndof, self.T
        if not 1 <= K <= 16 or B * K > 65535:
            raise ValueError("n_seeds must be in [1, 16] and B * n_seeds at most 65535")
        qc = np.ascontiguousarray(np.broadcast_to(np.asarray(qc, dtype=np.float64).reshape(-1, ndof), (B, ndof)))
        base = np.ascontiguousarray(np.broadcast_to(np.asarray(base_position, dtype=np.float64).reshape(-1, 3), (B, 3)))
        sid = self._scene_ids(fields, B)
        if int(h.opts.max_iter) != int(self.max_iter):
            h.set_opts(max_iter=int(self.max_iter))
        N, M = B * n_max, B * K
        slots = (B, K) if multi else (B,)  # leading shape of what exists once per solve instance
        f64, i32, u8 = torch.float64, torch.int32, torch.uint8
        res = SimpleNamespace()
        rs = None if retrieve is None else self.retrieve_spec(retrieve)
        hc = None  # the checked (clearance, cutoff, links) of a held_clearance request, before anything is enqueued
        if rs is not None and rs["held_clearance"] is not None:
            if rs["held_points"] is None:
                raise ValueError("retrieve: held_clearance needs held_points, the points it measures")
            hc = _capi.held_clearance_request(d, self.link_ee, rs["held_clearance"])
        convex = None  # (gap_tol, max_newton) when the retime dict asks for the grid's time optimum
        torque = None  # the checked tau_max and per-object payload arrays when it asks for torque limits on top
        if retime is not None and "profile" in retime:
            from ._capi import retime_profile
            prof = retime_profile(retime["profile"], retime.get("gap_tol", 1e-8), retime.get("max_newton"))
            convex = prof[1:] if prof[0] in ("convex", "torque") else None
            if prof[0] == "torque":  # checked here, before anything is enqueued
                from ._capi import payload_arrays, retime_torque_limits
                torque = dict(tau_max=retime_torque_limits(d, retime.get("tau_max")), payload=payload_arrays(retime.get("payload"), B))
        tr = None  # the checked controller and payload arrays of a track request, before anything is enqueued
        if track is not None:
            from ._capi import payload_arrays, track_controller
            from .gto_planner import TRACK_OPTIONS
            if retime is None:
                raise ValueError("plan_objects: track needs retime, the trajectories it rolls out")
            unknown = set(track) - (TRACK_OPTIONS - {"n_samples"})
            if unknown or "kp" not in track or "kd" not in track:
                raise TypeError(f"plan_objects: track needs kp and kd and takes {sorted(TRACK_OPTIONS - {'n_samples'})}, got {sorted(track)}")
            plant = track.get("plant_payload", retime.get("payload"))
            tr = dict(ctl={k: v for k, v in track.items() if not k.endswith("_payload")}, plant=payload_arrays(plant, B),
                      model=payload_arrays(track.get("model_payload", plant), B))
            track_controller(d, **tr["ctl"])

        def rollout(tag, M_ref, d_duration, d_samples, model, plant):
            """One gto_track_rollout_device behind the retime call that wrote d_duration and d_samples; returns its outputs."""
            outs = dict(err_max=self._dev(tag + "err_max", (B,), f64), err_end=self._dev(tag + "err_end", (B,), f64),
                        sat_steps=self._dev(tag + "sat_steps", (B,), i32), status=self._dev(tag + "status", (B,), i32))
            up = lambda kind, pl: [None if a is None else self._up(f"{tag}{kind}_{k}", a, np.float64).data_ptr()  # noqa: E731
                                   for k, a in zip(("mass", "com", "inertia"), pl)]
            h.track_rollout_device(B, M_ref, d_duration.data_ptr(), *[t.data_ptr() for t in d_samples], n_samples=2,
                                   model_payload=up("model", model), plant_payload=up("plant", plant),
                                   err_max=outs["err_max"].data_ptr(), err_end=outs["err_end"].data_ptr(),
                                   sat_steps=outs["sat_steps"].data_ptr(), status_out=outs["status"].data_ptr(), stream=st, **tr["ctl"])
            return {tag + k: v for k, v in outs.items()}

        sc = None if self_check is None else _capi.self_check_request(d, self_check)  # before anything is enqueued
        d_self = {}  # the per-column results of the self-clearance launches: prefix -> (d2, pair)

        def self_clearance(prefix, cols, d_paths):
            """One gto_self_clearance_device on the chain's stream behind whatever wrote d_paths (B, ndof, cols)."""
            d_d2, d_pair = self._dev(prefix + "d2_cols", (B, cols), f64), self._dev(prefix + "pair_cols", (B, cols, 2), i32)
            h.self_clearance_device(B, cols, d_paths.data_ptr(), d_d2.data_ptr(), d_pair.data_ptr(), cutoff=sc[1], stream=st)
            d_self[prefix] = (d_d2, d_pair)

        tracked = {}
        if sc is not None:
            h.set_self_pairs(sc[2])  # (a host fact of the handle: the launches below carry it as an argument)
        with torch.cuda.stream(self.stream):
            st = self.stream.cuda_stream
            d_sid, d_qc, d_base = self._up("sid", sid, np.int32), self._up("qc", qc, np.float64), self._up("base", base, np.float64)
            d_ikg, d_pg, d_ng, extra = feed(st, d_base)
            d_obj_pose = extra.pop("_object_pose", None)  # plan_grasps: the poses of the objects, which the robot then holds

            def upload_held():
                """The held object's points, counts, poses and labels -> device buffers of the chain (None: nothing to check)."""
                if rs is None or rs["held_points"] is None or (observation is None and hc is None):
                    return None
                pts, n_held = h.pad_held_points(rs["held_points"], rs["held_counts"])
                if pts.shape[0] != B or n_held.shape != (B,):
                    raise ValueError(f"retrieve: held_points needs one point set per object ({B})")
                held = SimpleNamespace(P_max=pts.shape[1], points=self._up("held_points", pts, np.float64),
                                       counts=self._up("held_counts", n_held, np.int32), pose=d_obj_pose, labels=None, label=None)
                if rs["object_pose"] is not None:
                    held.pose = self._up("held_pose", np.asarray(rs["object_pose"], dtype=np.float64).reshape(B, 16), np.float64)
                if rs["labels"] is not None:
                    held.labels = self._up("held_labels", np.asarray(rs["labels"]), np.int32)
                if rs["held_label"] is not None:
                    held.label = self._up("held_label", np.broadcast_to(np.asarray(rs["held_label"], dtype=np.int32), (B,)), np.int32)
                return held

            # per candidate grasp: its object's scene, seed and base
            d_sid_ik = self._up("sid_ik", np.repeat(sid, n_max), np.int32)
            d_q0_ik = self._up("q0_ik", np.repeat(qc, n_max, axis=0), np.float64)
            d_base_ik = self._up("base_ik", np.repeat(base, n_max, axis=0), np.float64)
            d_q = self._dev("q_sol", (B, n_max, ndof), f64)
            d_ikf, d_ikit, d_ikst = self._dev("ik_f", (B, n_max), f64), self._dev("ik_it", (B, n_max), i32), self._dev("ik_st", (B, n_max), i32)
            d_ep, d_er, d_ic = self._dev("err_pos", (B, n_max), f64), self._dev("err_rot", (B, n_max), f64), self._dev("ik_cost", (B, n_max), f64)
            d_acc = self._dev("accept", (B, n_max), u8)
            d_gc, d_ngc, d_nacc = self._dev("goals_c", slots + (n_max, 16), f64), self._dev("n_goals_c", slots, i32), self._dev("n_acc", (B,), i32)
            d_Q0, d_si = self._dev("Q0", slots + (ndof, T), f64), self._dev("seed_index", slots, i32)
            d_sc, d_sd = self._dev("seed_cost", (B, n_max), f64), self._dev("seed_dist", (B, n_max), f64)
            d_Q, d_dQ = self._dev("Q", (B, ndof, T), f64), self._dev("dQ", (B, ndof, T - 1), f64)
            d_f, d_it, d_stat = self._dev("f", slots, f64), self._dev("it", slots, i32), self._dev("stat", slots, i32)
            d_so = None
            if use_standoff:
                S = standoff_pose(self.standoff_distance, axis_standoff)
                d_so = self._up("standoff", np.broadcast_to(np.asarray(S, dtype=np.float64).reshape(1, 16), (M, 16)), np.float64)
            so_ptr = None if d_so is None else d_so.data_ptr()
            d_gc.zero_()  # rows behind an object's accepted goals are never read; they are defined all the same
            d_sc.fill_(float("nan"))
            d_sd.fill_(float("nan"))
            if multi:
                # per slot: its object's scene, current configuration and base; the slots' plans, of which d_Q gets the best
                base_s = np.repeat(base, K, axis=0)
                d_sid_s, d_qc_s = self._up("sid_slot", np.repeat(sid, K), np.int32), self._up("qc_slot", np.repeat(qc, K, axis=0), np.float64)
                d_base_s = self._up("base_slot", base_s, np.float64)
                d_Qs, d_dQs = self._dev("slot_Q", (B, K, ndof, T), f64), self._dev("slot_dQ", (B, K, ndof, T - 1), f64)
                d_rows = self._dev("accepted_rows", (B, n_max), i32)
                d_gi, d_gcost = self._dev("slot_goal_index", (B, K), i32), self._dev("slot_goal_cost", (B, K), f64)
                d_pep, d_per = self._dev("slot_err_pos", (B, K), f64), self._dev("slot_err_rot", (B, K), f64)
                d_scls, d_best, d_cls = self._dev("slot_class", (B, K), i32), self._dev("best_slot", (B,), i32), self._dev("plan_class", (B,), i32)
                d_rows.fill_(-1)
            d_cnt = None
            if N:
                h.solve_ik_pose_batch_device(0, N, d_sid_ik.data_ptr(), d_q0_ik.data_ptr(), d_ikg.data_ptr(), d_base_ik.data_ptr(),
                                             self.ik_max_iter, d_q.data_ptr(), d_ikf.data_ptr(), d_ikit.data_ptr(),
                                             d_ikst.data_ptr(), st)
                # behind the IK launch: the host's copies into pinned memory run while the GPU solves IK, and no copy is
                # enqueued behind the solve
                held = upload_held()
                h.ik_report_device(N, d_sid_ik.data_ptr(), d_q.data_ptr(), d_ikg.data_ptr(), d_base_ik.data_ptr(), pos_tol,
                                   rot_tol_deg, ik_collision_threshold, d_ep.data_ptr(), d_er.data_ptr(), d_ic.data_ptr(),
                                   d_acc.data_ptr(), st)
                seed_in = (d_sid.data_ptr(), d_qc.data_ptr(), d_pg.data_ptr(), d_ng.data_ptr(), d_q.data_ptr(), d_acc.data_ptr(),
                           d_base.data_ptr(), interpolate, float32_solutions, d_gc.data_ptr(), d_ngc.data_ptr(), d_nacc.data_ptr())
                seed_out = (d_Q0.data_ptr(), d_si.data_ptr(), d_sc.data_ptr(), d_sd.data_ptr(), st)
                if not multi:
                    h.seed_goalsets_device(B, n_max, *seed_in, *seed_out)
                    h.solve_batch_device(B, n_max, d_sid.data_ptr(), d_qc.data_ptr(), d_gc.data_ptr(), d_ngc.data_ptr(), so_ptr,
                                         d_base.data_ptr(), d_Q0.data_ptr(), d_Q.data_ptr(), d_dQ.data_ptr(), d_f.data_ptr(),
                                         d_it.data_ptr(), d_stat.data_ptr(), st)
                    if observation is not None:
                        d_cnt = self._dev("counts", (B, T), i32)
                        h.check_plans_device(observation, B, d_Q.data_ptr(), d_cnt.data_ptr(), base_pos=base, stream=st)
                else:
                    h.seed_goalsets_multi_device(B, n_max, K, *seed_in, d_rows.data_ptr(), *seed_out)
                    h.solve_batch_device(M, n_max, d_sid_s.data_ptr(), d_qc_s.data_ptr(), d_gc.data_ptr(), d_ngc.data_ptr(), so_ptr,
                                         d_base_s.data_ptr(), d_Q0.data_ptr(), d_Qs.data_ptr(), d_dQs.data_ptr(), d_f.data_ptr(),
                                         d_it.data_ptr(), d_stat.data_ptr(), st)
                    h.plan_report_device(M, n_max, d_gc.data_ptr(), d_ngc.data_ptr(), so_ptr, d_Qs.data_ptr(), d_gi.data_ptr(),
                                         d_gcost.data_ptr(), d_pep.data_ptr(), d_per.data_ptr(), st)
                    if observation is not None:
                        d_cnt = self._dev("counts", (B, K, T), i32)
                        h.check_plans_device(observation, M, d_Qs.data_ptr(), d_cnt.data_ptr(), base_pos=base_s, stream=st)
                    sel = (d_stat.data_ptr(), d_f.data_ptr(), d_pep.data_ptr(), d_per.data_ptr(),
                           None if d_cnt is None else d_cnt.data_ptr(), pos_tol, rot_tol_deg, int(max_points))
                    h.select_plans_device(M, 1, *sel, class_out=d_scls.data_ptr(), stream=st)  # every slot on its own: its class
                    h.select_plans_device(B, K, *sel, Q=d_Qs.data_ptr(), dQ=d_dQs.data_ptr(), best_slot_out=d_best.data_ptr(),
                                          class_out=d_cls.data_ptr(), Q_out=d_Q.data_ptr(), dQ_out=d_dQ.data_ptr(), stream=st)
                if sc is not None:  # the selected plan
                    self_clearance("self_", T, d_Q)
                if retrieve is not None:
                    lift = rs["mode"] == "lift"
                    cols = int(rs["steps"]) + 1 if lift else h.retrieve_path_columns()
                    if cols < 1:
                        raise ValueError("retrieve: the horizon is shorter than the stretch the reverse mode runs backwards")
                    d_rp = self._dev("retrieve_path", (B, ndof, cols), f64)
                    if lift:
                        d_rreach, d_rstat = self._dev("retrieve_reached", (B,), i32), self._dev("retrieve_status", (B, cols - 1), i32)
                        h.retrieve_lift_device(B, d_Q.data_ptr(), d_sid.data_ptr() if rs["collide"] else None, d_base.data_ptr(),
                                               rs["direction"], rs["distance"], rs["steps"], rs["closed_joints"], rs["closed_value"],
                                               self.ik_max_iter, pos_tol, rot_tol_deg, d_rp.data_ptr(), status_out=d_rstat.data_ptr(),
                                               reached_out=d_rreach.data_ptr(), stream=st)
                    else:
                        h.retrieve_reverse(B, d_Q.data_ptr(), rs["closed_joints"], rs["closed_value"], d_rp.data_ptr(), stream=st)
                    if sc is not None:
                        self_clearance("retrieve_self_", cols, d_rp)
                    if observation is not None:
                        d_rcnt = self._dev("retrieve_counts", (B, cols), i32)
                        h.check_paths_device(observation, B, cols, d_rp.data_ptr(), d_rcnt.data_ptr(), base_pos=base, stream=st)
                        if held is not None:  # the object rides with link_ee from the grasp: the plan's last waypoint
                            ptr = lambda t: None if t is None else t.data_ptr()
                            d_hcnt = self._dev("retrieve_held_counts", (B, cols), i32)
                            h.check_held_paths_device(observation, B, cols, d_rp.data_ptr(), held.points.data_ptr(), held.P_max,
                                                      held.counts.data_ptr(), d_hcnt.data_ptr(), attach=None if lift else d_Q.data_ptr(),
                                                      attach_ld=T, attach_col=T - 1, object_pose=ptr(held.pose), labels=ptr(held.labels),
                                                      held_label=ptr(held.label), base_pos=base, stream=st)
                    if hc is not None:  # the object against the arm that carries it: needs no observation
                        d_hc = (self._dev("retrieve_held_self_d2_cols", (B, cols), f64), self._dev("retrieve_held_self_link_cols", (B, cols), i32),
                                self._dev("retrieve_held_self_point_cols", (B, cols), i32))
                        h.held_clearance_device(B, cols, d_rp.data_ptr(), held.points.data_ptr(), held.P_max, held.counts.data_ptr(),
                                                *[t.data_ptr() for t in d_hc], attach=None if lift else d_Q.data_ptr(), attach_ld=T,
                                                attach_col=T - 1, object_pose=None if held.pose is None else held.pose.data_ptr(),
                                                base_pos=base, links=hc[2], cutoff=hc[1], stream=st)
                if retime is not None:
                    d_dur, d_rst = self._dev("durations", (B,), f64), self._dev("retime_status", (B,), i32)
                    samp = {}  # the approach's samples, kept only for the rollout
                    if tr is not None:
                        d_tsamp = [self._dev("track_ref_" + k, (B, int(retime.get("n_samples", 100)), ndof), f64) for k in ("q", "qd", "qdd")]
                        samp = {k + "_out": v.data_ptr() for k, v in zip(("q", "qd", "qdd"), d_tsamp)}
                    if convex is None:
                        h.retime_batch_device(B, d_Q.data_ptr(), retime["vmax"], retime["amax"], int(retime.get("subdiv", 2)),
                                              int(retime.get("n_samples", 100)), duration_out=d_dur.data_ptr(),
                                              status_out=d_rst.data_ptr(), stream=st, **samp)
                    elif torque is not None:  # the approach: the hand is empty
                        d_rit = self._dev("retime_iters", (B,), i32)
                        h.retime_paths_torque_device(B, T, d_Q.data_ptr(), retime["vmax"], retime["amax"], tau_max=torque["tau_max"],
                                                     subdiv=int(retime.get("subdiv", 2)), n_samples=int(retime.get("n_samples", 100)),
                                                     gap_tol=convex[0], max_newton=convex[1], duration_out=d_dur.data_ptr(),
                                                     status_out=d_rst.data_ptr(), iters_out=d_rit.data_ptr(), stream=st, **samp)
                    else:  # the plans are the Tp = T case of the paths call
                        d_rit = self._dev("retime_iters", (B,), i32)
                        h.retime_paths_convex_device(B, T, d_Q.data_ptr(), retime["vmax"], retime["amax"],
                                                     subdiv=int(retime.get("subdiv", 2)), n_samples=int(retime.get("n_samples", 100)),
                                                     gap_tol=convex[0], max_newton=convex[1], duration_out=d_dur.data_ptr(),
                                                     status_out=d_rst.data_ptr(), iters_out=d_rit.data_ptr(), stream=st, **samp)
                    if tr is not None:  # the approach: the hand is empty, and the controller knows it
                        tracked.update(rollout("track_", int(retime.get("n_samples", 100)), d_dur, d_tsamp, (None,) * 3, (None,) * 3))
                    if retrieve is not None:  # the retrieve path on the same clock rules, behind the retrieve stage
                        sub, ns = int(retime.get("subdiv", 2)), int(retime.get("n_samples", 100))
                        d_nc = None
                        if lift and rs["reached_only"]:
                            d_nc = self._dev("retrieve_n_cols", (B,), i32)
                            torch.add(d_rreach, 1, out=d_nc)
                        d_rdur, d_rrst = self._dev("retrieve_durations", (B,), f64), self._dev("retrieve_retime_status", (B,), i32)
                        d_rsamp, d_rtau = [None] * 3, None
                        if retime.get("retrieve_samples", False):
                            d_rsamp = [self._dev("retrieve_" + k, (B, ns, ndof), f64) for k in ("q", "qd", "qdd")]
                        d_rref = d_rsamp  # what the rollout reads: the caller's samples, or buffers of the chain's own
                        if tr is not None and d_rsamp[0] is None:
                            d_rref = [self._dev("retrieve_track_ref_" + k, (B, ns, ndof), f64) for k in ("q", "qd", "qdd")]
                        outs = dict(duration_out=d_rdur.data_ptr(), status_out=d_rrst.data_ptr(),
                                    **{k + "_out": None if v is None else v.data_ptr() for k, v in zip(("q", "qd", "qdd"), d_rref)})
                        if convex is None:
                            h.retime_paths_device(B, cols, d_rp.data_ptr(), retime["vmax"], retime["amax"],
                                                  n_cols=None if d_nc is None else d_nc.data_ptr(), subdiv=sub, n_samples=ns,
                                                  **outs, stream=st)
                        elif torque is not None:  # the retrieve motion carries each object's payload
                            d_rrit = self._dev("retrieve_retime_iters", (B,), i32)
                            d_pl = [None if a is None else self._up("retime_payload_" + k, a, np.float64).data_ptr()
                                    for k, a in zip(("mass", "com", "inertia"), torque["payload"])]
                            if d_rsamp[0] is not None:
                                d_rtau = self._dev("retrieve_tau", (B, ns, ndof), f64)
                            h.retime_paths_torque_device(B, cols, d_rp.data_ptr(), retime["vmax"], retime["amax"],
                                                         tau_max=torque["tau_max"], payload_mass=d_pl[0], payload_com=d_pl[1],
                                                         payload_inertia=d_pl[2], n_cols=None if d_nc is None else d_nc.data_ptr(),
                                                         subdiv=sub, n_samples=ns, gap_tol=convex[0], max_newton=convex[1],
                                                         iters_out=d_rrit.data_ptr(), tau_out=None if d_rtau is None else d_rtau.data_ptr(),
                                                         **outs, stream=st)
                        else:
                            d_rrit = self._dev("retrieve_retime_iters", (B,), i32)
                            h.retime_paths_convex_device(B, cols, d_rp.data_ptr(), retime["vmax"], retime["amax"],
                                                         n_cols=None if d_nc is None else d_nc.data_ptr(), subdiv=sub, n_samples=ns,
                                                         gap_tol=convex[0], max_newton=convex[1], iters_out=d_rrit.data_ptr(),
                                                         **outs, stream=st)
                        if tr is not None:  # the object is in the hand now
                            tracked.update(rollout("retrieve_track_", ns, d_rdur, d_rref, tr["model"], tr["plant"]))
            out = dict(plans=d_Q, dQ=d_dQ, cost=d_f, iters=d_it, status=d_stat, n_accepted=d_nacc, seed_index=d_si, seed_cost=d_sc,
                       seed_dist=d_sd, q_solutions=d_q, err_pos=d_ep, err_rot=d_er, ik_cost=d_ic, ik_iters=d_ikit, ik_status=d_ikst,
                       accept=d_acc)
            out.update(extra)
            out.update(tracked)
            for prefix, (d_d2, d_pair) in d_self.items():
                out["_" + prefix + "d2_cols"], out["_" + prefix + "pair_cols"] = d_d2, d_pair
            if d_cnt is not None:
                out["counts"] = d_cnt
            if N and retime is not None:
                out["durations"], out["retime_status"] = d_dur, d_rst
                if convex is not None:
                    out["retime_iters"] = d_rit
            if N and retrieve is not None:
                out["retrieve_path"] = d_rp
                if lift:
                    out["retrieve_reached"], out["retrieve_status"] = d_rreach, d_rstat
                if observation is not None:
                    out["retrieve_counts"] = d_rcnt
                    if held is not None:
                        out["retrieve_held_counts"] = d_hcnt
                if hc is not None:
                    out["_held_d2_cols"], out["_held_link_cols"], out["_held_point_cols"] = d_hc
                if retime is not None:
                    out["retrieve_durations"], out["retrieve_retime_status"] = d_rdur, d_rrst
                    if convex is not None:
                        out["retrieve_retime_iters"] = d_rrit
                    out.update({"retrieve_" + k: v for k, v in zip(("q", "qd", "qdd"), d_rsamp) if v is not None})
                    if d_rtau is not None:
                        out["retrieve_tau"] = d_rtau
            if multi:  # (cost, iters, status and counts hold every slot's until the chosen slot's are picked below)
                out.update(best_slot=d_best, plan_class=d_cls, slot_class=d_scls, slot_goal_index=d_gi, slot_err_pos=d_pep,
                           slot_err_rot=d_per, accepted_rows=d_rows, slot_plans=d_Qs)
            host = {k: self._pin("out/" + k, v.shape, v.dtype) for k, v in out.items()}
            for k, v in out.items():
                host[k].copy_(v, non_blocking=True)
        self.stream.synchronize()  # the one host synchronisation of the call
        for k, v in host.items():
            if not k.startswith("_"):
                setattr(res, k, v.numpy().copy())
        for prefix in d_self:  # per plan: the closest column's d2 and pair, and whether every column is clear
            found = _capi.self_check_summary(host["_" + prefix + "d2_cols"].numpy(), host["_" + prefix + "pair_cols"].numpy(), sc[0], prefix)
            for k, v in found.items():
                setattr(res, k, v.copy())
        if "_held_d2_cols" in host:  # per plan: the closest column of the held object against the robot's own links
            found = _capi.held_clearance_summary(*[host[f"_held_{k}_cols"].numpy() for k in ("d2", "link", "point")], hc[0],
                                                 "retrieve_held_self_")
            for k, v in found.items():
                setattr(res, k, v.copy())
        res.accept = res.accept.astype(bool)
        if float32_solutions:
            res.q_solutions = res.q_solutions.astype(np.float32)
        if N and retrieve is not None and not lift:  # every column of the reversed stretch is the plan's own
            res.retrieve_reached = np.full(B, cols, dtype=np.int32)
            res.retrieve_status = np.zeros((B, 0), dtype=np.int32)
        if multi:  # the chosen slot's entries of the small per-slot arrays, picked on the host
            rows, best = np.arange(B), res.best_slot
            res.slot_cost, res.slot_iters, res.slot_status = res.cost, res.iters, res.status
            res.cost, res.iters, res.status = res.slot_cost[rows, best], res.slot_iters[rows, best], res.slot_status[rows, best]
            res.goal_index = res.slot_goal_index[rows, best]
            res.plan_err_pos, res.plan_err_rot = res.slot_err_pos[rows, best], res.slot_err_rot[rows, best]
            if hasattr(res, "counts"):
                res.slot_counts = res.counts
                res.counts = res.slot_counts[rows, best]
            known = (res.n_accepted > 0) & (res.goal_index >= 0)
            res.goal_row = np.where(known, res.accepted_rows[rows, np.maximum(res.goal_index, 0)], -1).astype(np.int32)
        return res
