"""The motion after the grasp (include/gto_solver.h gto_retrieve_lift / gto_retrieve_reverse_device), restated on the host.

lift_chain is a Python loop over a solver with the surface of oracle.Oracle (eval_fk, solve_ik_batch): RT0 from eval_fk, the
goals in numpy, then solve_ik_batch K times, each step seeded from the one before.  With the FP64 oracle it is the reference
the fused kernel is held to; with a SolverHandle it is the same chain driven from the host, one launch and one round trip per
step, which the fused kernel has to reproduce bit for bit.  reverse_path is the shelf branch as a numpy index expression.
"""
import numpy as np

from helpers import cfg_of
from grasptrajopt_amd.robot_desc import load_builtin

POS_TOL, ROT_TOL_DEG = 0.01, 5.0  # the driver's acceptance test (examples/pybullet_gto_planning.py:262)
MAX_ITER = 50                     # gto/ik_solver.py:76
STATUS_CONVERGED, STATUS_MAX_ITER, STATUS_NUMERICAL = 0, 1, 2


def finger_joints(desc):
    """The parameter joints that are fingers: what the driver closes (cfg['finger_index'])."""
    return [int(i) for i in desc.param_index if "finger" in desc.actuated_joint_names[int(i)]]


def column0(plans, closed_joints, closed_values):
    """(B, ndof): the plans' last waypoints with the closed joints' entries replaced."""
    q = np.array(plans, dtype=np.float64)[:, :, -1].copy()
    if len(closed_joints):
        q[:, np.asarray(closed_joints, dtype=np.int64)] = np.broadcast_to(np.asarray(closed_values, dtype=np.float64), (len(closed_joints),))
    return q


def lift_goals(RT0, distance, K, direction):
    """(B, K, 4, 4): RT0's rotation, translation p0[a] + (k * (distance / K)) * direction[a] -- one rounding per operation,
    as numpy computes it."""
    RT0 = np.asarray(RT0, dtype=np.float64).reshape(-1, 4, 4)
    direction = np.asarray(direction, dtype=np.float64).reshape(3)
    goals = np.repeat(RT0[:, None], K, axis=1).copy()
    step = np.float64(distance) / np.float64(K)
    for k in range(1, K + 1):
        s = np.float64(k) * step
        goals[:, k - 1, :3, 3] = RT0[:, :3, 3] + s * direction
    return goals


def pose_errors(RT, T_ee):
    """err_pos, err_rot (degrees) of gto/ik_solver.py:88-97 as gto_ik_report_device states them."""
    RT, T_ee = np.asarray(RT).reshape(-1, 4, 4), np.asarray(T_ee).reshape(-1, 4, 4)
    ep = np.linalg.norm(RT[:, :3, 3] - T_ee[:, :3, 3], axis=1)
    tr = np.einsum("bij,bij->b", RT[:, :3, :3], T_ee[:, :3, :3])
    return ep, np.degrees(np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0)))


def lift_chain(solver, desc, link_ee, plans, distance, K, direction=(0.0, 0.0, 1.0), closed_joints=(), closed_values=0.0,
               scene_id=None, base_pos=None, max_iter=MAX_ITER, pos_tol=POS_TOL, rot_tol_deg=ROT_TOL_DEG):
    """The chain of gto_retrieve_lift driven step by step through ``solver`` -> dict of path (B, ndof, K + 1), goals
    (B, K, 4, 4), iters, status, err_pos, err_rot (B, K) and reached (B,)."""
    fe = desc.frame_index(link_ee)
    q = column0(plans, closed_joints, closed_values)
    B = q.shape[0]
    goals = lift_goals(solver.eval_fk(q)[:, fe], distance, K, direction)
    path = np.empty((B, desc.ndof, K + 1))
    path[:, :, 0] = q
    iters, status = np.empty((B, K), dtype=np.int32), np.empty((B, K), dtype=np.int32)
    err_pos, err_rot = np.empty((B, K)), np.empty((B, K))
    for k in range(1, K + 1):
        q, _, iters[:, k - 1], status[:, k - 1] = solver.solve_ik_batch(scene_id, q, goals[:, k - 1].reshape(B, 16), base_pos, max_iter=max_iter)
        path[:, :, k] = q
        err_pos[:, k - 1], err_rot[:, k - 1] = pose_errors(goals[:, k - 1], solver.eval_fk(q)[:, fe])
    ok = (err_pos < pos_tol) & (err_rot < rot_tol_deg) & (status != STATUS_NUMERICAL)
    reached = np.cumprod(ok, axis=1).sum(axis=1).astype(np.int32)
    return dict(path=path, goals=goals, iters=iters, status=status, err_pos=err_pos, err_rot=err_rot, reached=reached)


def reverse_path(plans, standoff_offset=-10, closed_joints=(), closed_values=0.0):
    """examples/pybullet_gto_planning.py:310-312: plan[:, arange(standoff_offset - 10, -1)][:, ::-1], finger rows closed."""
    plans = np.asarray(plans, dtype=np.float64)
    T = plans.shape[2]
    if T + standoff_offset - 10 < 0:
        raise ValueError("the horizon is shorter than the stretch the reference reverses")
    out = plans[:, :, np.arange(standoff_offset - 10, -1)][:, :, ::-1].copy()
    if len(closed_joints):
        out[:, np.asarray(closed_joints, dtype=np.int64), :] = np.broadcast_to(
            np.asarray(closed_values, dtype=np.float64), (len(closed_joints),))[None, :, None]
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs
LIFT = {"panda": 0.2, "fetch": 0.2}  # metres: within reach of every grasp configuration below (test_retrieve_cpu checks it)


def grasp_plans(robot, B, T=50, seed=0):
    """(desc, cfg, plans (B, ndof, T)): seeded plans that end in in-limit grasp configurations around the robot's default pose
    with the fingers open; the columns before the last are a straight joint-space approach from the default pose."""
    desc, cfg = load_builtin(robot), cfg_of(robot)
    rng = np.random.default_rng(1234 + 17 * seed + (0 if robot == "panda" else 5))
    q0 = np.asarray(cfg["default_pose"], dtype=np.float64)
    opt = np.asarray(desc.opt_index, dtype=np.int64)
    qg = np.tile(q0, (B, 1))
    lo, hi = desc.lower[opt], desc.upper[opt]
    qg[:, opt] = np.clip(q0[opt] + rng.uniform(-0.25, 0.25, size=(B, len(opt))), lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo))
    fingers = finger_joints(desc)
    qg[:, fingers] = np.asarray(cfg["gripper_open_offsets"], dtype=np.float64)
    s = np.linspace(0.0, 1.0, T)
    plans = q0[None, :, None] + (qg - q0)[:, :, None] * s[None, None, :]
    plans[:, fingers, :] = qg[:, fingers, None]
    return desc, cfg, np.ascontiguousarray(plans)


# A thin cost board over the grasp poses, for the chains that run with the collision term: zero up to 5 cm above the mean
# hand height, a 10 cm ramp up to `amp`, 25 cm thick, 24 cm wide.  The hand and the wrist links meet it while they are
# lifted.  The amplitude is small on purpose: the term enters the step through its gradient alone, and on a redundant arm a
# strong field moves the null space by radians per step; at 1e-5 the chain still differs from the field-free one by tenths
# of a radian and a 1e-12 change of the input moves it by about 1e-11 (measured on the oracle), so that a comparison at
# 1e-6 rad tests the arithmetic and not the conditioning.
BOARD_AMP, BOARD_HALF, BOARD_POOL = 1e-5, 0.12, 24
# plans of the pool of 24 (seed 0) whose oracle chain through the board converges at every step within 30 iterations
BOARD_PLANS = {"panda": [5, 13, 19], "fetch": [2, 11, 16]}
BOARD_MAX_ITERS = 30


def board(center, zc, amp=BOARD_AMP, half=BOARD_HALF, n=48, res=0.05, origin=(-1.0, -1.2, -0.4)):
    """(c_all, c_obs, shape, origin, res) of the board around (center[0], center[1]) from height zc on."""
    ax = [origin[a] + res * np.arange(n) for a in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    ramp = np.clip((Z - zc) / 0.1, 0, 1) * np.clip((zc + 0.25 - Z) / 0.1, 0, 1)
    lat = np.clip((half - np.abs(X - center[0])) / 0.1, 0, 1) * np.clip((half - np.abs(Y - center[1])) / 0.1, 0, 1)
    f = (amp * ramp * lat).astype(np.float32)
    return f, f, (n, n, n), np.asarray(origin, dtype=np.float64), res


def board_case(robot, fk):
    """(desc, cfg, plans (3, ndof, T), scene): the plans of BOARD_PLANS and the board over the pool's mean hand position;
    ``fk`` is an eval_fk (the oracle's: the scene must not depend on the code under test)."""
    desc, cfg, pool = grasp_plans(robot, BOARD_POOL, seed=0)
    p = fk(pool[:, :, -1])[:, desc.frame_index(cfg["link_ee"]), :3, 3]
    return desc, cfg, np.ascontiguousarray(pool[BOARD_PLANS[robot]]), board(p.mean(axis=0), p[:, 2].mean() + 0.05)
