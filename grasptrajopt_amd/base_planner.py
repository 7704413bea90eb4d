"""BasePlanner — drop-in for the reference's gto/base_planner.py, solved on the GPU.

The reference builds an OpTaS problem with T = goal_size (gto/base_planner.py:35-94): a planar base pose
(x, y, theta) shared by all goals, one arm configuration per goal, gripper point matching against
``tf_base @ RT_i @ gripper_tf``, an effort term on the base pose, joint limits and |theta| <= pi, and hands
it to IPOPT (max_iter 100).  Here the same objective goes through ``gto_solve_base_batch``: one workgroup
per goal set runs the whole projected Levenberg-Marquardt iteration on the MI355X, and several goal sets
(the resampling loop of examples/pybullet_gto_planning_mobile.py:185-199) can be solved in ONE call.

``place_base`` is that resampling loop itself on one stream: many draws of grasps go in, ``gto_solve_base_batch_device`` ->
``gto_base_report_device`` place the base for every draw, report the errors and count the robot's footprint on the resident
occupancy grid, and the first draw whose footprint is free comes out after ONE host synchronisation.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from .utils import rotZ


class BasePlanner:
    def __init__(self, robot, link_ee, link_gripper):
        self.robot = robot
        self.robot_name = robot.get_name()
        self.link_ee = link_ee
        self.link_gripper = link_gripper
        self.gripper_points = robot.surface_pc_map[link_gripper].points
        self.task_name = "base_pose_estimator"  # gto/base_planner.py:23
        self.max_iter = 100  # gto/base_planner.py:95
        self.goal_size = 1
        self.base_effort_weight = 0.01
        self._handle = None
        self._buf = {}
        self._stream = None

    def setup_optimization(self, goal_size=1, base_effort_weight=0.01):
        """gto/base_planner.py:35-96: nothing symbolic to build; records the sizes and binds the handle."""
        self.goal_size = int(goal_size)
        self.base_effort_weight = float(base_effort_weight)
        self._handle = self.robot.solver_handle(self.link_ee, self.link_gripper, role="base")
        self._fe = self.robot.desc.frame_index(self.link_ee)
        self._fg = self.robot.desc.frame_index(self.link_gripper)

    # ------------------------------------------------------------------ batched entry point
    def plan_goalset_batch(self, qc, RTs_sets, n_goals=None):
        """B goal sets ``RTs_sets (B, n, 4, 4)`` (ragged through ``n_goals (B,)``) from configuration(s) ``qc``.
        Returns (Q (B, ndof, n), y (B, 3), err_pos (B, n), err_rot_deg (B, n), iters (B,), status (B,))."""
        if self._handle is None:
            self.setup_optimization(np.asarray(RTs_sets).shape[1], self.base_effort_weight)
        h, ndof = self._handle, self.robot.ndof
        RTs_sets = np.asarray(RTs_sets, dtype=np.float64)
        B, n = RTs_sets.shape[:2]
        qc = np.broadcast_to(np.asarray(qc, dtype=np.float64).reshape(-1, ndof), (B, ndof))
        y, q, _, iters, status = h.solve_base_batch(qc, RTs_sets, n_goals, self.base_effort_weight, self.max_iter)
        # errors as the reference reports them (gto/base_planner.py:127-143)
        fr = h.eval_fk(q.reshape(B * n, ndof)).reshape(B, n, -1, 4, 4)
        tf = fr[:, :, self._fg]
        G = np.linalg.inv(fr[:, :, self._fe]) @ tf
        RT_base = np.stack([_base_matrix(v) for v in y])
        RT = RT_base[:, None] @ RTs_sets @ G
        err_pos = np.linalg.norm(RT[..., :3, 3] - tf[..., :3, 3], axis=-1).astype(np.float32)
        cosang = (np.einsum("bnij,bnij->bn", RT[..., :3, :3], tf[..., :3, :3]) - 1.0) / 2.0  # = 2 (q1.q2)^2 - 1
        err_rot = np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0))).astype(np.float32)
        return np.transpose(q, (0, 2, 1)).copy(), y, err_pos, err_rot, iters, status

    def base_collision_cost(self, qc, y):
        """gto/base_planner.py:146-158: robot surface points at qc, seen from the moved base, summed over the
        x-y occupancy grid (robot.setup_occupancy_grid)."""
        if not hasattr(self.robot, "occupancy_grid"):
            raise RuntimeError("call robot.setup_occupancy_grid(points) before planning the base")
        RT_base_inv = np.linalg.inv(_base_matrix(y))
        pts, _ = self.robot.compute_fk_surface_points(np.asarray(qc, dtype=np.float64).reshape(-1), tf_base=RT_base_inv)
        offsets = self.robot.points_to_offsets_occupancy_numpy(pts)
        return float(np.sum(self.robot.occupancy_grid[offsets]))

    # ------------------------------------------------------------------ the resampling loop, stream-ordered
    @staticmethod
    def draw_goal_sets(RTs_by_object, num=2, draws=64, rng=None, indices=None):
        """The goal sets of ``draws`` passes of the driver's sampling (examples/pybullet_gto_planning_mobile.py:163-181): ``num``
        random rows of every object that has any grasp, concatenated in object order.  ``indices (draws, n_objects, num)``
        overrides the sampling (the entries of an object without grasps are ignored).  Returns (goal sets (draws, n, 4, 4),
        the indices used)."""
        objs = [np.asarray(r, dtype=np.float64).reshape(-1, 4, 4) for r in RTs_by_object]
        if indices is None:
            rng = np.random.default_rng() if rng is None else rng
            indices = np.zeros((draws, len(objs), num), dtype=np.int64)
            for d in range(draws):
                for o, r in enumerate(objs):
                    if len(r):
                        indices[d, o] = rng.integers(0, len(r), size=num)
        indices = np.asarray(indices, dtype=np.int64)
        if indices.ndim != 3 or indices.shape[1] != len(objs):
            raise ValueError(f"indices must be (draws, {len(objs)}, num), got {indices.shape}")
        sets = [np.concatenate([r[indices[d, o]] for o, r in enumerate(objs) if len(r)]) for d in range(indices.shape[0])]
        return np.stack(sets) if sets else np.zeros((0, 0, 4, 4)), indices

    def _dev(self, name, shape, dtype):
        """A device buffer of the planner, kept between calls while the shape stays (grasp_chain.GraspChain._dev)."""
        t = self._buf.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = self._torch.empty(tuple(shape), dtype=dtype, device=self._device)
            self._buf[name] = t
        return t

    def _pin(self, name, shape, dtype):
        """A pinned host buffer of the planner (a call ends with a synchronisation: nothing is in flight when it is reused)."""
        t = self._buf.get("pin/" + name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = self._torch.empty(tuple(shape), dtype=dtype, pin_memory=True)
            self._buf["pin/" + name] = t
        return t

    def _up(self, name, array, dtype):
        """Host array -> the planner's device buffer of that name, through pinned memory, on the current stream."""
        src = self._torch.from_numpy(np.require(array, dtype=dtype, requirements=["C", "W"]))
        pin = self._pin(name, src.shape, src.dtype)
        pin.copy_(src)
        dst = self._dev(name, src.shape, src.dtype)
        dst.copy_(pin, non_blocking=True)
        return dst

    def place_base(self, qc, RTs_by_object, num=2, draws=64, rng=None, indices=None, occupancy=None):
        """The driver's ``while 1: sample grasps -> plan_goalset -> if cost == 0: break`` (:185-199) for ``draws`` draws at
        once.  RTs_by_object: per object its grasp poses (n_o, 4, 4) in the current base frame; the goal sets are drawn by
        ``draw_goal_sets``.  occupancy: an occupancy.OccupancyGrid (default: the one ``robot.setup_occupancy_grid`` left on
        the robot when it was given device-resident points).

        Returns a namespace: draw (the first draw whose footprint is free, -1: none, the caller asks again), plan (ndof, n),
        y (3,), err_pos (n,), err_rot (n,) float32 and cost of that draw (of draw 0 when there is none), collision (draws,)
        (the reference's cost of every draw; -1: a non-finite placement), iters, status (draws,), indices."""
        import torch
        occ = occupancy if occupancy is not None else getattr(self.robot, "occupancy", None)
        if occ is None:
            raise RuntimeError("place_base needs a resident occupancy grid: pass occupancy=OccupancyGrid... or call "
                               "robot.setup_occupancy_grid(DepthPointCloud.points)")
        goals, indices = self.draw_goal_sets(RTs_by_object, num, draws, rng, indices)
        B, n = goals.shape[:2]
        if B == 0 or n == 0:
            raise ValueError("place_base: no draw or no grasp to place the base for")
        if self._handle is None or self.goal_size != n:
            self.setup_optimization(n, self.base_effort_weight)
        h, ndof = self._handle, self.robot.ndof
        if self._stream is None:
            self._torch = torch
            self._device = torch.device("cuda", occ.device)
            self._stream = torch.cuda.Stream(device=self._device)
        qc = np.ascontiguousarray(np.broadcast_to(np.asarray(qc, dtype=np.float64).reshape(-1, ndof), (B, ndof)))
        ng = np.full(B, n, dtype=np.int32)
        f64, i32, i64 = torch.float64, torch.int32, torch.int64
        with torch.cuda.stream(self._stream):
            st = self._stream.cuda_stream
            d_qc, d_goals = self._up("qc", qc, np.float64), self._up("goals", goals.reshape(B, n, 16), np.float64)
            d_y, d_q = self._dev("y", (B, 3), f64), self._dev("q", (B, n, ndof), f64)
            d_it, d_stat = self._dev("it", (B,), i32), self._dev("stat", (B,), i32)
            d_ep, d_er = self._dev("err_pos", (B, n), f64), self._dev("err_rot", (B, n), f64)
            d_col, d_ff = self._dev("collision", (B,), i32), self._dev("first_free", (1,), i32)
            h.solve_base_batch_device(B, n, ng, d_qc.data_ptr(), d_goals.data_ptr(), self.base_effort_weight, self.max_iter,
                                      d_y.data_ptr(), d_q.data_ptr(), None, d_it.data_ptr(), d_stat.data_ptr(), st)
            h.base_report_device(occ, B, n, ng, d_qc.data_ptr(), d_goals.data_ptr(), d_y.data_ptr(), d_q.data_ptr(),
                                 d_ep.data_ptr(), d_er.data_ptr(), d_col.data_ptr(), d_ff.data_ptr(), st)
            pick = d_ff.to(i64).clamp_(min=0)  # the chosen draw's rows alone come back (draw 0 when none is free)
            out = dict(first_free=d_ff, collision=d_col, iters=d_it, status=d_stat, y=d_y.index_select(0, pick),
                       q=d_q.index_select(0, pick), err_pos=d_ep.index_select(0, pick), err_rot=d_er.index_select(0, pick))
            host = {k: self._pin("out/" + k, v.shape, v.dtype) for k, v in out.items()}
            for k, v in out.items():
                host[k].copy_(v, non_blocking=True)
        self._stream.synchronize()  # the one host synchronisation of the call
        res = SimpleNamespace(draw=int(host["first_free"][0]), indices=indices)
        k = max(res.draw, 0)
        res.collision, res.iters, res.status = (host[a].numpy().copy() for a in ("collision", "iters", "status"))
        res.plan = host["q"].numpy()[0].T.copy()
        res.y = host["y"].numpy()[0].copy()
        res.err_pos, res.err_rot = host["err_pos"].numpy()[0].astype(np.float32), host["err_rot"].numpy()[0].astype(np.float32)
        res.cost = float(res.collision[k])
        return res

    # ------------------------------------------------------------------ reference signature
    def plan_goalset(self, qc, RTs):
        """gto/base_planner.py:97-165 -> (Q (ndof, n), y (3,), err_pos (n,), err_rot_deg (n,), collision cost)."""
        RTs = np.asarray(RTs, dtype=np.float64).reshape(-1, 4, 4)
        Q, y, err_pos, err_rot, _, _ = self.plan_goalset_batch(np.asarray(qc, dtype=np.float64).reshape(1, -1), RTs[None])
        cost = self.base_collision_cost(qc, y[0])
        return Q[0], y[0], err_pos[0], err_rot[0], cost


def _base_matrix(y):
    """RT_base of gto/base_planner.py:122-125."""
    M = rotZ(y[2])
    M[0, 3], M[1, 3] = y[0], y[1]
    return M
