"""GTOPlanner — same constructor and plan()/plan_goalset() signatures and return values as the
reference (gto/gto_planner.py:21-245); the solve runs on the MI355X solver behind the C ABI."""
from __future__ import annotations

import numpy as np

from . import optas_facade as optas
from .synthetic import standoff_pose
from .utils import interpolate_waypoints


# the keys of a track= request: the keywords of utils.track_trajectories
TRACK_OPTIONS = frozenset(("kp", "kd", "tau_max", "dt", "settle", "n_samples", "feedforward", "model_payload", "plant_payload", "locked"))


class GTOPlanner:
    def __init__(self, robot, link_ee, link_gripper, collision_avoidance=True, standoff_distance=-0.1,
                 standoff_offset=-10):
        self.T = 50          # gto/gto_planner.py:25
        self.Tmax = 10.0     # :26
        self.dt = self.Tmax / (self.T - 1)  # :27-28
        self.standoff_offset = standoff_offset
        self.standoff_distance = standoff_distance
        self.robot = robot
        self.robot_name = robot.get_name()
        self.link_ee = link_ee
        self.link_gripper = link_gripper
        self.gripper_points = robot.surface_pc_map[link_gripper].points
        self.collision_avoidance = collision_avoidance
        self.max_iter = 100  # :141

    def setup_optimization(self, goal_size=1, use_standoff=False, axis_standoff="x"):
        """gto/gto_planner.py:42-142 with structured cost terms instead of CasADi expressions."""
        builder = optas.OptimizationBuilder(T=self.T, robots=[self.robot])
        builder.add_parameter("qc", self.robot.ndof)
        builder.add_parameter("tf_goal", 16, goal_size)
        builder.add_parameter("sdf_cost_all", self.robot.field_size)
        builder.add_parameter("sdf_cost_obstacle", self.robot.field_size)
        builder.add_parameter("base_position", 3)
        builder.initial_configuration(self.robot_name)
        builder.initial_configuration(self.robot_name, time_deriv=1)
        builder.integrate_model_states(self.robot_name, time_deriv=1, dt=self.dt)
        self.pose_standoff = standoff_pose(self.standoff_distance, axis_standoff)
        builder.add_cost_term("cost_pos", optas.GoalSetPointMatching(
            self.link_ee, self.link_gripper, goal_size, bool(use_standoff), self.pose_standoff, self.standoff_offset))
        if self.collision_avoidance:
            builder.add_cost_term("cost_obstacle", optas.ObstacleField(10.0, self.standoff_offset))
        builder.add_cost_term("min_join_vel", optas.JointVelocity(0.01))
        builder.enforce_model_limits(self.robot_name)
        solver_options = {"ipopt": {"max_iter": self.max_iter, "tol": 1e-15}}
        self.solver = optas.CasADiSolver(builder.build()).setup("ipopt", solver_options=solver_options)

    def _seed_from(self, qc, q_solution):
        data = interpolate_waypoints(np.stack([qc, q_solution]), self.T, self.robot.ndof)
        index = np.array(self.robot.parameter_joint_indexes).astype(np.int32)
        data[:, index] = np.array(qc)[index]
        return data.T

    def plan(self, qc, RT, sdf_cost_obstacle, base_position, q_solution=None, use_standoff=True, axis_standoff="x"):
        """gto/gto_planner.py:145-182.  As in the reference, ``sdf_cost_all`` is not passed here and
        therefore defaults to zeros for the waypoints before the standoff."""
        if hasattr(sdf_cost_obstacle, "resident"):  # a field that is resident on the device: its scene (and with it the grid
            sdf_cost_obstacle.resident()          # geometry the problem is sized by) before anything else
        self.setup_optimization(goal_size=1, use_standoff=use_standoff, axis_standoff=axis_standoff)
        qc = np.asarray(qc, dtype=np.float64)
        tf_goal = np.zeros((16, 1))
        tf_goal[:, 0] = np.asarray(RT, dtype=np.float64).flatten()
        if q_solution is None:
            Q0 = np.diag(qc) @ np.ones((self.robot.ndof, self.T))
        else:
            Q0 = self._seed_from(qc, np.asarray(q_solution, dtype=np.float64))
        self.solver.reset_initial_seed({f"{self.robot_name}/q/x": self.robot.extract_optimized_dimensions(Q0)})
        self.solver.reset_parameters({
            "qc": qc, "tf_goal": tf_goal, "sdf_cost_obstacle": sdf_cost_obstacle, "base_position": base_position,
            f"{self.robot_name}/q/p": self.robot.extract_parameter_dimensions(Q0)})
        solution = self.solver.solve()
        return (solution[f"{self.robot_name}/q"].toarray(), solution[f"{self.robot_name}/dq"].toarray(),
                solution["f"].toarray().flatten())

    def plan_goalset(self, qc, RTs, sdf_cost_all, sdf_cost_obstacle, base_position, q_solutions=None,
                     use_standoff=True, axis_standoff="x", interpolate=True):
        """gto/gto_planner.py:185-245."""
        for fld in (sdf_cost_obstacle, sdf_cost_all):  # fields that are resident on the device: their scene (and with it the
            if hasattr(fld, "resident"):               # grid geometry the problem is sized by) before anything else; the
                fld.resident()                         # obstacle field first: its build holds both fields
        RTs = np.asarray(RTs, dtype=np.float64)
        qc = np.asarray(qc, dtype=np.float64)
        n = RTs.shape[0]
        self.setup_optimization(goal_size=n, use_standoff=use_standoff, axis_standoff=axis_standoff)
        tf_goal = np.zeros((16, n))
        for i in range(n):
            tf_goal[:, i] = RTs[i].flatten()
        # parameters first: the parameter-joint rows of every seed are qc's (gto/gto_planner.py:204-205,234), so the
        # dictionary does not depend on the seed, and the scene is uploaded ONCE for seed scoring and solve
        qp = np.tile(qc[np.array(self.robot.parameter_joint_indexes, dtype=np.int64)][:, None], (1, self.T))
        self.solver.reset_parameters({
            "qc": qc, "tf_goal": tf_goal, "sdf_cost_all": sdf_cost_all, "sdf_cost_obstacle": sdf_cost_obstacle,
            "base_position": base_position, f"{self.robot_name}/q/p": qp})
        if q_solutions is None:
            Q0 = np.diag(qc) @ np.ones((self.robot.ndof, self.T))
        else:
            # seed = interpolation towards the IK solution with the lowest obstacle cost, ties broken by
            # joint distance (gto/gto_planner.py:197-215); all candidates are scored in one GPU call against
            # c_obs of the scene the solve uses
            q_solutions = np.asarray(q_solutions, dtype=np.float64)
            plans = np.stack([self._seed_from(qc, q_solutions[:, i]) for i in range(q_solutions.shape[1])])
            sid = self.solver.ensure_scene()
            cost_all, dist_all = self.solver._handle.plan_cost(sid, plans, base_position)
            self.seed_cost_all, self.seed_dist_all = cost_all, dist_all
            ind = np.lexsort((dist_all, cost_all))
            self.seed_index = int(ind[0])
            if interpolate:
                Q0 = plans[ind[0]]
            else:
                Q0 = np.diag(qc) @ np.ones((self.robot.ndof, self.T))
                for i in range(self.T + self.standoff_offset, self.T):
                    Q0[:, i] = plans[ind[0]][:, self.T - 1]
        self.solver.reset_initial_seed({f"{self.robot_name}/q/x": self.robot.extract_optimized_dimensions(Q0)})
        solution = self.solver.solve()
        return (solution[f"{self.robot_name}/q"].toarray(), solution[f"{self.robot_name}/dq"].toarray(),
                solution["f"].toarray().flatten())

    def self_clearance(self, plan, clearance=None, cutoff=None, mask=None, q_ref=None):
        """The robot's distance from itself at every waypoint of a solved ``plan`` (ndof, T) or (B, ndof, T):
        ``utils.self_clearance`` (dict d2, dist, pair, clear).  The solve has no self-collision term: a plan whose wrist
        passes through the base is found here, not by the solver."""
        from .utils import self_clearance
        return self_clearance(self.robot, plan, clearance=clearance, cutoff=cutoff, mask=mask, q_ref=q_ref)

    def retrieve_path(self, plan, mode="lift", distance=0.3, steps=10, direction=(0.0, 0.0, 1.0), closed_joints=None,
                      closed_value=0.0, max_iter=50, pos_tol=0.01, rot_tol_deg=5.0, retime=None, observation=None,
                      held_points=None, n_held=None, object_pose=None, labels=None, held_label=None,
                      base_position=(0.0, 0.0, 0.0), track=None, self_check=None, held_clearance=None):
        """The motion after the grasp (examples/pybullet_gto_planning.py:301-313) for a solved ``plan`` (ndof, T), or
        (B, ndof, T) for B of them: mode "lift" moves link_ee by ``distance`` along ``direction`` in ``steps`` IK steps, each
        seeded from the one before, with the gripper's pose held (the tabletop driver's env.retract; pybullet's position-only
        IK would let the held object tilt); mode "reverse" runs the plan's last stretch backwards (the shelf driver).
        ``closed_joints`` (default: the robot's parameter joints that are fingers) are held at ``closed_value``.
        Returns (path (ndof, steps + 1 | 9 - standoff_offset), reached): reached counts the leading steps that met their goal
        within pos_tol / rot_tol_deg (reverse: every column).  No collision term; GraspChain's ``retrieve`` has one.
        retime: a dict ``vmax, amax[, subdiv, n_samples, reached_only, profile, gap_tol, max_newton, tau_max, payload]`` to
        also retime the path under these joint limits (gto_retime_paths; ``profile="convex"``: the grid's time optimum,
        gto_retime_paths_convex, whose dict also has ``iters``; ``profile="torque"``: that optimum under the joint torque limits
        ``tau_max`` (None: the description's effort limits) with the held object ``payload`` on link_ee, the dict of
        ``utils.inverse_dynamics``, gto_retime_paths_torque, whose dict also has ``tau``); reached_only=True retimes columns 0 .. reached of a lift, the part that met its goals.  The
        return value is then (path, reached, trajectory): the dict of ``SolverHandle.retime_paths`` (of one path for one
        plan).
        observation + held_points: the points of the object the robot holds (per plan (n_i, 3) world points at the moment of
        the grasp, or a padded array with n_held; object-frame points with object_pose (4, 4) per plan) are carried with
        link_ee along the path from the grasp configuration -- the plan's last waypoint, which is column 0 of a lift
        and is not part of a reversed path -- and counted inside ``observation`` at every column
        (gto_check_held_paths; labels / held_label: the segmentation image of a depth observation and the held object's
        label).  The return value then ends with one more element, the dict ``{"held_counts": (columns,) | (B, columns)}``.
        track: a dict ``kp, kd[, tau_max, dt, settle, n_samples, feedforward, model_payload, plant_payload, locked]`` (the
        keywords of ``utils.track_trajectories``) to also roll the retimed trajectory forward under that joint controller
        (gto_track_rollout); it needs ``retime``.  model_payload and plant_payload default to the retime's payload, on
        link_ee.  The trajectory dict gains ``track_q, track_qd, track_t, track_err_max, track_err_end, track_sat_steps,
        track_steps, track_status``.
        self_check: a dict ``[clearance, cutoff, mask, q_ref]`` (``_capi.self_check_request``; {} for the defaults) to also
        measure the robot's clearance from itself along the path (gto_self_clearance).  The dict at the end of the return
        value -- the one that holds held_counts, added if there is none -- gains ``self_d2`` (the smallest squared distance
        over the columns), ``self_pair`` (2,) and ``self_clear`` per plan.
        held_clearance: a dict ``[clearance, cutoff, links, ignore]`` (``_capi.held_clearance_request``; {} for the defaults)
        to also measure the held points' clearance from the robot's own links along the path (gto_held_clearance): the
        object against the arm that carries it.  It needs ``held_points`` and no observation (without one the counts are
        not computed and ``held_counts`` is absent).  The dict at the end of the return value gains ``held_self_d2`` (the
        smallest squared distance over the columns), ``held_self_col``, ``held_self_link``, ``held_self_point`` and
        ``held_self_clear`` per plan."""
        from . import _capi
        from .grasp_chain import finger_joints
        plan = np.asarray(plan, dtype=np.float64)
        single = plan.ndim == 2
        plans = np.ascontiguousarray(plan.reshape(-1, self.robot.ndof, self.T))
        if self_check is not None:  # checked before the handle is made
            self_check = _capi.self_check_request(self.robot.desc, self_check)
        if held_clearance is not None:
            if held_points is None:
                raise ValueError("retrieve_path: held_clearance needs held_points, the points it measures")
            held_clearance = _capi.held_clearance_request(self.robot.desc, self.link_ee, held_clearance)
        torque = None  # a torque request is checked before the handle is made: (tau_max, payload dict)
        if retime is not None and retime.get("profile") == "torque":
            _capi.payload_arrays(retime.get("payload"), plans.shape[0])
            torque = (_capi.retime_torque_limits(self.robot.desc, retime.get("tau_max")), retime.get("payload"))
        if track is not None:  # checked before the handle is made, like the torque request
            if retime is None:
                raise ValueError("retrieve_path: track needs retime, the trajectory it rolls out")
            unknown = set(track) - TRACK_OPTIONS
            if unknown or "kp" not in track or "kd" not in track:
                raise TypeError(f"retrieve_path: track needs kp and kd and takes {sorted(TRACK_OPTIONS)}, got {sorted(track)}")
            track = dict(track)
            for k in ("model_payload", "plant_payload"):
                track.setdefault(k, retime.get("payload"))
                _capi.payload_arrays(track[k], plans.shape[0])
            _capi.track_controller(self.robot.desc, **{k: v for k, v in track.items() if not k.endswith("_payload")})
        opts = _capi.default_opts()
        opts.T, opts.Tmax, opts.standoff_offset = self.T, self.Tmax, self.standoff_offset
        h = self.robot.solver_handle(self.link_ee, self.link_gripper, opts, role="retrieve")
        closed = finger_joints(self.robot.desc) if closed_joints is None else closed_joints
        if mode == "lift":
            out = h.retrieve_lift(plans, distance, steps, direction, closed, closed_value, max_iter=max_iter, pos_tol=pos_tol,
                                  rot_tol_deg=rot_tol_deg)
            path, reached = out["path"], out["reached"]
        elif mode == "reverse":
            import torch
            n = h.retrieve_path_columns()
            if n < 1:
                raise ValueError("retrieve_path: the horizon is shorter than the stretch the reverse mode runs backwards")
            dev = torch.device("cuda", self.robot.device)
            d_plans = torch.from_numpy(plans).to(dev)
            d_path = torch.empty((plans.shape[0], self.robot.ndof, n), dtype=torch.float64, device=dev)
            stream = torch.cuda.current_stream(dev)
            h.retrieve_reverse(plans.shape[0], d_plans.data_ptr(), closed, closed_value, d_path.data_ptr(), stream=stream.cuda_stream)
            path = d_path.cpu().numpy()  # (synchronises the stream)
            reached = np.full(plans.shape[0], n, dtype=np.int32)
        else:
            raise ValueError('retrieve_path: mode is "lift" or "reverse"')
        checks = ()
        if held_points is not None:
            if observation is None and held_clearance is None:
                raise ValueError("retrieve_path: held_points need the observation they are counted in")
            B = plans.shape[0]
            if single and n_held is None and isinstance(held_points, np.ndarray) and held_points.ndim == 2:
                held_points = [held_points]
            # a lift starts at the grasp (its column 0); a reversed path leaves that column out: the plan's last waypoint
            attach = plans if mode == "reverse" else None
            pose = None if object_pose is None else np.broadcast_to(np.asarray(object_pose, dtype=np.float64).reshape(-1, 16), (B, 16))
            base = np.asarray(base_position, dtype=np.float64)
            found = {}
            if observation is not None:
                from .observation import as_observation
                counts = h.check_held_paths(as_observation(observation), path, held_points, n_held=n_held, attach=attach,
                                            object_pose=pose, labels=labels, held_label=held_label, base_pos=base)
                found["held_counts"] = counts[0] if single else counts
            if held_clearance is not None:
                hc = h.held_clearance(path, held_points, n_held=n_held, attach=attach, object_pose=pose, base_pos=base,
                                      links=held_clearance[2], cutoff=held_clearance[1])
                summary = _capi.held_clearance_summary(hc["d2"], hc["link"], hc["point"], held_clearance[0])
                found.update({k: v[0] if single else v for k, v in summary.items()})
            checks = (found,)
        if self_check is not None:
            h.set_self_pairs(self_check[2])
            sc = h.self_clearance(path, cutoff=self_check[1])
            found = _capi.self_check_summary(sc["d2"], sc["pair"], self_check[0])
            checks = (dict(checks[0] if checks else {}, **{k: v[0] if single else v for k, v in found.items()}),)
        if retime is None:
            return ((path[0], int(reached[0])) if single else (path, reached)) + checks
        unknown = set(retime) - {"vmax", "amax", "subdiv", "n_samples", "reached_only", "profile", "gap_tol", "max_newton", "tau_max", "payload"}
        if unknown:
            raise TypeError(f"retrieve_path: unexpected retime key(s) {sorted(unknown)}")
        n_cols = reached + 1 if mode == "lift" and retime.get("reached_only", False) else None
        profile, gap_tol, max_newton = _capi.retime_profile(retime.get("profile", "greedy"), retime.get("gap_tol", 1e-8),
                                                            retime.get("max_newton"))
        kw = dict(n_cols=n_cols, subdiv=int(retime.get("subdiv", 2)), n_samples=int(retime.get("n_samples", 100)))
        if profile == "torque":
            traj = h.retime_paths_torque(path, retime["vmax"], retime["amax"], tau_max=torque[0], payload=torque[1],
                                         gap_tol=gap_tol, max_newton=max_newton, **kw)
        elif profile == "convex":
            traj = h.retime_paths_convex(path, retime["vmax"], retime["amax"], gap_tol=gap_tol, max_newton=max_newton, **kw)
        else:
            traj = h.retime_paths(path, retime["vmax"], retime["amax"], **kw)
        if track is not None:
            rolled = h.track_rollout(traj["duration"], traj["q"], traj["qd"], traj["qdd"], **track)
            traj.update({"track_" + k: v for k, v in rolled.items()})
        return ((path[0], int(reached[0]), {k: v[0] for k, v in traj.items()}) if single else (path, reached, traj)) + checks
