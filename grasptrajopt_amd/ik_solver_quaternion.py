"""IKSolver — drop-in for the reference's gto/ik_solver_quaternion.py, solved on the GPU.

The reference's T = 1 OpTaS problem (gto/ik_solver_quaternion.py:30-77) matches link_ee's position and unit quaternion
against ``tf_goal = (x, y, z, qx, qy, qz, qw)`` of the goal pose (:81-84):
``|p - g[:3]|^2 + 1 - (quat . g[3:])^2`` (:50-55), plus ``10 * sum(sdf_cost_obstacle[offsets])`` and the URDF joint
limits, IPOPT max_iter 50.  Here it goes through ``gto_solve_ik_pose_batch(GTO_IK_GOAL_QUATERNION)`` (DESIGN.md,
"Orientation-goal IK"); ``solve_ik_batch`` solves many goal poses in one call.
"""
from __future__ import annotations

from ._ik_pose import PoseIKSolver
from .utils import ik_goal_quaternion


class IKSolver(PoseIKSolver):
    GOAL_KIND = 1  # GTO_IK_GOAL_QUATERNION
    tf_goal = staticmethod(ik_goal_quaternion)

    def setup_optimization(self):
        """gto/ik_solver_quaternion.py:30-77: nothing symbolic to build; binds the solver handle."""
        super().setup_optimization()
