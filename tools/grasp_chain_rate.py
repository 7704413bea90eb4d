#!/usr/bin/env python3
"""grasp_chain_rate.py — time of the per-object loop of the reference's driver (examples/pybullet_gto_planning.py:242-294),
host-composed against stream-ordered, on identical inputs in one process on one MI355X: Panda-5k, a scene of about 128^3
voxels, 64 candidate grasps per object, 1 / 8 / 64 objects.

    baseline   per object: IKSolver.solve_ik_batch + the :262 filter in numpy + GTOPlanner.plan_goalset (cost fields passed
               as arrays, so every call uploads the scene to the IK handle and to the planner handle, as the parent does)
    chain      GraspChain.plan_objects over all objects with the same arrays (one upload per call)
    chain/res  GraspChain.plan_objects with the scene bound once (GraspChain.bind_scene) and named by its id

Plans, accepted sets and seed indices are compared before anything is timed.  Median of five timed regions after one
warm-up region, the two paths alternating; a region ends with the device synchronised (both paths end in one).
    python tools/grasp_chain_rate.py [--commit TEXT] [--objects 1,8,64] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (lib_sha16)
import grasptrajopt_amd as g  # noqa: E402
from grasptrajopt_amd import synthetic as syn  # noqa: E402
from grasptrajopt_amd.grasp_chain import GraspChain  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--commit", default="unknown")
ap.add_argument("--objects", default="1,8,64")
ap.add_argument("--grasps", type=int, default=64)
ap.add_argument("--out", default=None)
a = ap.parse_args()

with open(os.path.join(ROOT, "grasptrajopt_amd", "data", "panda_cfg.json")) as fh:
    cfg = json.load(fh)
robot = g.GTORobotModel(desc=g.load_builtin("panda_5k"), time_derivs=[0, 1], param_joints=cfg["param_joints"],
                        collision_link_names=cfg["collision_link_names"], device=0)
robot.grid_resolution = 2.4 / 128  # a 1.6 m cloud + 0.4 m margin on either side: about 128 voxels per axis
rng = np.random.default_rng(0)
robot.setup_points_field(rng.uniform([-0.4, -0.8, -0.4], [1.2, 0.8, 1.2], size=(4000, 3)))
wp = robot.workspace_points
qd = np.abs(wp - np.array([0.55, 0.1, 0.1])) - np.array([0.06, 0.06, 0.1])
d_box = np.linalg.norm(np.maximum(qd, 0), axis=1) + np.minimum(qd.max(axis=1), 0)
d_table = wp[:, 2] + 0.1  # a table top 10 cm below the robot's base: the base link stays out of its cost band
c_all = syn.sdf_cost_map(np.minimum(d_table, d_box), epsilon=0.06).astype(np.float32)
c_obs = syn.sdf_cost_map(d_table, epsilon=0.06).astype(np.float32)
shape = robot.field_geometry()[0]
n = a.grasps
ik = g.IKSolver(robot, cfg["link_ee"], cfg["link_gripper"], collision_avoidance=True)
planner = g.GTOPlanner(robot, cfg["link_ee"], cfg["link_gripper"], standoff_distance=-0.1, standoff_offset=-10)
chain = GraspChain(robot, cfg["link_ee"], cfg["link_gripper"], standoff_distance=-0.1, standoff_offset=-10)
chain.bind_scene(5, c_all, c_obs)
qc = np.array(cfg["default_pose"], dtype=np.float64)
base = np.zeros(3)
THR = 5.0


def baseline(RT):
    out = []
    for b in range(RT.shape[0]):
        q, ep, er, cost, _, _ = ik.solve_ik_batch(qc, RT[b], c_obs, base)
        found = (ep < 0.01) & (er < 5.0) & (cost < THR)
        if not found.any():
            out.append((found, None, -1))
            continue
        plan, _, _ = planner.plan_goalset(qc, RT[b][found], c_all, c_obs, base, q.T.astype(np.float32)[:, found], use_standoff=True,
                                          axis_standoff=cfg["axis_standoff"], interpolate=True)
        out.append((found, plan, planner.seed_index))
    return out


def new(RT, fields):
    return chain.plan_objects(qc, RT, RT, np.full(RT.shape[0], n, np.int32), fields, base, axis_standoff=cfg["axis_standoff"],
                              ik_collision_threshold=THR)


def timed(fns, reps=5):
    for f in fns:
        f()  # warm-up
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):  # alternating
            t0 = time.perf_counter()
            f()
            ts[i].append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(t), min(t), max(t)) for t in ts]


lines = [f"# tools/grasp_chain_rate.py on one MI355X; commit {a.commit}, lib_sha16 {bench.lib_sha16()}",
         f"# Panda-5k ({robot.desc.n_points} points), scene {shape[0]}x{shape[1]}x{shape[2]}, {n} grasps per object, T 50, solve cap 100, IK cap 50",
         "# ms per region, median of 5 [min .. max] after one warm-up, paths alternating; a region ends synchronised",
         "# baseline: per object IKSolver.solve_ik_batch + numpy filter + GTOPlanner.plan_goalset (arrays: two scene uploads per object)",
         "# chain: GraspChain.plan_objects, same arrays (one scene upload per call); chain/res: scene bound once"]
for B in [int(x) for x in a.objects.split(",")]:
    RT, _ = syn.make_goals(robot.desc, robot._util_handle().eval_fk, cfg["link_ee"], B * n, seed=100 + B, zlim=(0.15, 0.6))
    RT = RT.reshape(B, n, 4, 4)
    want, got, got_r = baseline(RT), new(RT, (c_all, c_obs)), new(RT, 5)
    same = all(np.array_equal(w[0], got.accept[b]) and w[2] == got.seed_index[b] and (w[1] is None or w[1].tobytes() == got.plans[b].tobytes())
               for b, w in enumerate(want)) and got.plans.tobytes() == got_r.plans.tobytes()
    assert same and got.accept.any(), "the two paths differ, or no grasp was accepted: nothing to time"
    t = timed([lambda: baseline(RT), lambda: new(RT, (c_all, c_obs)), lambda: new(RT, 5)])
    lines.append(f"objects {B:3d}   baseline {t[0][0]:9.3f} ms [{t[0][1]:.3f} .. {t[0][2]:.3f}]   chain {t[1][0]:9.3f} ms [{t[1][1]:.3f} .. {t[1][2]:.3f}]   "
                 f"chain/res {t[2][0]:9.3f} ms [{t[2][1]:.3f} .. {t[2][2]:.3f}]   baseline/chain x{t[0][0] / t[1][0]:.2f}   baseline/chain-res x{t[0][0] / t[2][0]:.2f}")
    lines.append(f"    plans, accepted sets and seed indices equal: {same}; accepted {int(got.accept.sum())} of {B * n}; objects without a grasp {int((got.n_accepted == 0).sum())}")
    print("\n".join(lines[-2:]), flush=True)
text = "\n".join(lines) + "\n"
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
chain.close()
robot.close()
