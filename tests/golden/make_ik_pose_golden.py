#!/usr/bin/env python3
"""Generate tests/golden/ik_pose.npz by EXECUTING THE REFERENCE'S OWN PYTHON numerics (optas/models.py
get_global_link_quaternion / get_global_link_rpy, optas/spatialmath.py Quaternion.getrpy / fromrpy) through the numpy
stand-ins of _reference_stubs.py, in the style of make_golden.py.  Build-container only; the .npz (data only) is what
the tests read.  Re-run:  python tests/golden/make_ik_pose_golden.py

The pose terms are those of gto/ik_solver_quaternion.py:50-55 (|p - g[:3]|^2 + 1 - (quat . g[3:])^2, tf_goal of
:81-84) and gto/ik_solver_rpy.py:53-58 (|p - g[:3]|^2 + |(rpy - g[3:]) / pi|^2, tf_goal of :84-89), evaluated on the
reference's quaternion and angles.  The stand-in casadi module lacks the few functions getrpy and the cost use
(atan2, asin, fabs, if_else, dot); they are added to it here at run time.

Per robot (Panda, Fetch): about 64 random in-limit configurations, a few whose link_ee pitch is near +-pi/2 and at
least one exactly on the clamp |sin(pitch)| >= 1 (found with the oracle's FK, then evaluated by the reference), the
link_ee position / quaternion / rpy of each, goal vectors built from other configurations, and the reference's
pose-term value of (configuration, goal) pairs.
"""
import itertools
import os
import sys

import numpy as np
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import _reference_stubs as stubs  # noqa: E402

REF = stubs.REF


def _add_casadi_functions():
    cs = sys.modules["casadi"]
    cs.atan2 = lambda y, x: np.arctan2(np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64))
    cs.asin = lambda x: np.arcsin(np.clip(np.asarray(x, dtype=np.float64), -1.0, 1.0))  # (the branch if_else discards)
    cs.fabs = lambda x: np.abs(np.asarray(x, dtype=np.float64))
    cs.if_else = lambda c, a, b: np.where(np.asarray(c, dtype=bool), a, b)
    cs.dot = lambda a, b: float(np.dot(np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()))


def _flat(a):
    return np.asarray(a, dtype=np.float64).ravel()


def clamp_and_near_configs(robot, cfg, n_near):
    """Configurations whose link_ee has |R20| = 1 exactly (pitch on the clamp) and ones just off it, found with the
    oracle's FK (only the choice of configurations; every stored number comes from the reference)."""
    from grasptrajopt_amd.robot_desc import load_builtin
    from oracle import oracle
    d = load_builtin(robot)
    o = oracle.Oracle(d, cfg["link_ee"], cfg["link_gripper"])
    fe = d.frame_index(cfg["link_ee"])
    qc = np.array(cfg["default_pose"], dtype=np.float64)
    oi = d.opt_index
    cands = [0.0, np.pi / 2, -np.pi / 2]
    last = cands + [np.pi / 4, -np.pi / 4, 3 * np.pi / 4, -3 * np.pi / 4]  # (Panda's hand sits at -pi/4 on its flange)
    clamp = []
    for combo in itertools.product(*([cands] * (len(oi) - 1) + [last])):
        q = qc.copy()
        q[oi] = combo
        if np.any(q[oi] < d.lower[oi]) or np.any(q[oi] > d.upper[oi]):
            continue
        R20 = o.eval_fk(q[None])[0, fe, 2, 0]
        if abs(R20) >= 1.0:
            clamp.append(q)
    seeds = clamp
    if not clamp:  # none exactly on it: the closest ones seed the near-clamp search
        Q = []
        for combo in itertools.product(*([cands] * (len(oi) - 1) + [last])):
            q = qc.copy()
            q[oi] = combo
            if not (np.any(q[oi] < d.lower[oi]) or np.any(q[oi] > d.upper[oi])):
                Q.append(q)
        Q = np.array(Q)
        seeds = [Q[i] for i in np.argsort(1.0 - np.abs(o.eval_fk(Q)[:, fe, 2, 0]))[:n_near]]
    # near the clamp: 1 - |R20| = delta, by bisection on the second-last optimised joint from a clamp configuration
    near = []
    for q in seeds[:n_near]:
        for delta in (1e-3, 1e-6):
            j = oi[-2]
            lo_, hi_ = q[j], min(q[j] + 0.5, d.upper[oi][-2])
            f = lambda t: 1.0 - abs(o.eval_fk(np.concatenate([q[:j], [t], q[j + 1:]])[None])[0, fe, 2, 0]) - delta
            if f(hi_) <= 0:
                continue
            for _ in range(200):
                m = 0.5 * (lo_ + hi_)
                lo_, hi_ = (m, hi_) if f(m) < 0 else (lo_, m)
            qn = q.copy()
            qn[j] = hi_
            near.append(qn)
    return clamp, near


def golden_pose(ref, robot, rng):
    cfg = yaml.safe_load(open(f"{REF}/data/configs/{robot}.yaml"))["robot_cfg"]
    import json
    lcfg = json.load(open(os.path.join(ROOT, "grasptrajopt_amd", "data", f"{robot}_cfg.json")))
    m = ref.models.RobotModel(urdf_filename=f"{REF}/{cfg['urdf_robot_path']}", time_derivs=[0, 1],
                              param_joints=cfg["param_joints"])
    ee = cfg["link_ee"]
    lo = np.asarray(m.lower_actuated_joint_limits).ravel()
    hi = np.asarray(m.upper_actuated_joint_limits).ravel()
    lo_c, hi_c = np.maximum(lo, -3.2), np.minimum(hi, 3.2)
    q = rng.uniform(lo_c, hi_c, size=(64, m.ndof))
    q[0] = np.array(cfg["default_pose"])
    clamp, near = clamp_and_near_configs(robot, lcfg, 2)
    clamp = clamp[:2]
    q = np.concatenate([q] + [np.array(c).reshape(-1, m.ndof) for c in (clamp, near)])
    kind_of = np.array([0] * 64 + [2] * len(clamp) + [1] * len(near), dtype=np.int32)  # 0 random, 1 near, 2 on the clamp
    Q = ref.spatialmath.Quaternion
    nq = len(q)
    pos, quat, rpy, rpy_of_quat = np.zeros((nq, 3)), np.zeros((nq, 4)), np.zeros((nq, 3)), np.zeros((nq, 3))
    for i in range(nq):
        pos[i] = _flat(np.asarray(m.get_global_link_transform(ee, q[i]))[:3, 3])
        quat[i] = _flat(m.get_global_link_quaternion(ee, q[i]))
        rpy[i] = _flat(m.get_global_link_rpy(ee, q[i]))
        rpy_of_quat[i] = _flat(Q(*quat[i]).getrpy())  # Quaternion.getrpy on its own (the host's tf_goal path)
    # fromrpy: the quaternion of the reference's fixed-joint rotations (composition pinned through quat above)
    rpy_samples = rng.uniform(-np.pi, np.pi, size=(8, 3))
    fromrpy = np.array([_flat(Q.fromrpy(r).getquat()) for r in rpy_samples])
    # goals from FK of other configurations; the reference's pose terms of (configuration, goal) pairs
    perm = rng.permutation(nq)
    gq = np.concatenate([pos[perm], quat[perm]], axis=1)
    gq[1::3, 3:] *= 1.3  # (the reference does not normalise the goal quaternion)
    gr = np.concatenate([pos[perm], rpy[perm]], axis=1)
    f_quat, f_rpy = np.zeros(nq), np.zeros(nq)
    for i in range(nq):
        d = pos[i] - gq[i, :3]
        f_quat[i] = float(d @ d) + 1.0 - ref.models.cs.dot(quat[i], gq[i, 3:]) * ref.models.cs.dot(quat[i], gq[i, 3:])
        d = pos[i] - gr[i, :3]
        e = (rpy[i] - gr[i, 3:]) / np.pi
        f_rpy[i] = float(d @ d) + float(e @ e)
    return dict(q=q, kind=kind_of, pos=pos, quat=quat, rpy=rpy, rpy_of_quat=rpy_of_quat, rpy_samples=rpy_samples,
                fromrpy=fromrpy, goal_quat=gq, goal_rpy=gr, f_quat=f_quat, f_rpy=f_rpy)


def main():
    ref = stubs.install()
    _add_casadi_functions()
    rng = np.random.default_rng(20261016)
    out = {}
    for robot in ("panda", "fetch"):
        for k, v in golden_pose(ref, robot, rng).items():
            out[f"{robot}_{k}"] = v
    np.savez_compressed(f"{HERE}/ik_pose.npz", **out)
    print("ik_pose.npz", os.path.getsize(f"{HERE}/ik_pose.npz"))


if __name__ == "__main__":
    main()
