"""Shared body of the orientation-goal IK solvers (ik_solver_quaternion, ik_solver_rpy): the T = 1 problem of
gto/ik_solver.py with link_ee's position plus an orientation term as the pose term, solved on the GPU by
``gto_solve_ik_pose_batch`` (one workgroup per goal runs the whole projected Levenberg-Marquardt loop)."""
from __future__ import annotations

import numpy as np

from . import ik_solver, utils


class PoseIKSolver(ik_solver.IKSolver):
    GOAL_KIND = None  # include/gto_solver.h GTO_IK_GOAL_*

    @staticmethod
    def tf_goal(RT) -> np.ndarray:
        raise NotImplementedError

    def solve_ik_batch(self, q_0, RTs, sdf_cost_obstacle=None, base_position=None):
        """B seeds ``q_0 (B, ndof)`` (or one seed for all) and goal poses ``RTs (B, 4, 4)`` of link_ee.
        Returns (q (B, ndof), err_pos (B,), err_rot_deg (B,), cost (B,), iters (B,), status (B,))."""
        if self._handle is None:
            self.setup_optimization()
        h = self._handle
        RTs = np.asarray(RTs, dtype=np.float64).reshape(-1, 4, 4)
        B = RTs.shape[0]
        q_0 = np.broadcast_to(np.asarray(q_0, dtype=np.float64).reshape(-1, self.robot.ndof), (B, self.robot.ndof))
        base = np.zeros(3) if base_position is None else np.asarray(base_position, dtype=np.float64).reshape(3)
        sid = self._bind_scene(sdf_cost_obstacle)
        goals = np.stack([self.tf_goal(RT) for RT in RTs]) if B else np.zeros((0, 7 if self.GOAL_KIND == 1 else 6))
        q, f, iters, status = h.solve_ik_pose_batch(self.GOAL_KIND, sid, q_0, goals, base, self.max_iter)
        # errors as the reference reports them (gto/ik_solver_quaternion.py:98-103, gto/ik_solver_rpy.py:104-109)
        tf = h.eval_fk(q)[:, self._fe]
        err_pos = np.linalg.norm(RTs[:, :3, 3] - tf[:, :3, 3], axis=1)
        d = np.array([np.dot(utils.mat2quat(RTs[i, :3, :3]), utils.mat2quat(tf[i, :3, :3])) for i in range(B)])
        err_rot = np.arccos(np.clip(2 * np.square(d) - 1, -1, 1)) * 180 / np.pi
        return q, err_pos, err_rot, self._plan_cost(sid, q, base), iters, status

    def solve_ik(self, q_0, RT, sdf_cost_obstacle=None, base_position=None):
        """-> (q (ndof,), err_pos, err_rot_deg, cost), the reference's tuple."""
        q, ep, er, c, _, _ = self.solve_ik_batch(np.asarray(q_0, dtype=np.float64).reshape(1, -1), np.asarray(RT)[None],
                                                 sdf_cost_obstacle, base_position)
        return q[0], float(ep[0]), float(er[0]), float(c[0])
