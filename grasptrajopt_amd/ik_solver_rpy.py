"""IKSolver — drop-in for the reference's gto/ik_solver_rpy.py, solved on the GPU.

The reference's T = 1 OpTaS problem (gto/ik_solver_rpy.py:30-80) matches link_ee's position and roll-pitch-yaw angles
against ``tf_goal = (x, y, z, roll, pitch, yaw)`` of the goal pose (:84-89, the angles of optas Quaternion.getrpy):
``|p - g[:3]|^2 + |(rpy - g[3:]) / pi|^2`` (:53-58), plus ``10 * sum(sdf_cost_obstacle[offsets])`` and the URDF joint
limits, IPOPT max_iter 50.  As in the reference the angles are not wrapped: the term jumps where yaw or roll crosses
+-pi, and pitch is +pi/2 on both sides of the clamp |sin(pitch)| >= 1.  Here it goes through
``gto_solve_ik_pose_batch(GTO_IK_GOAL_RPY)`` ("Orientation-goal IK").
"""
from __future__ import annotations

from ._ik_pose import PoseIKSolver
from .utils import ik_goal_rpy


class IKSolver(PoseIKSolver):
    GOAL_KIND = 2  # GTO_IK_GOAL_RPY
    tf_goal = staticmethod(ik_goal_rpy)

    def setup_optimization(self):
        """gto/ik_solver_rpy.py:30-80: nothing symbolic to build; binds the solver handle."""
        super().setup_optimization()
