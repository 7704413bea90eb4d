#!/usr/bin/env python3
"""collision_check_rate.py — time of the collision checks against a resident observation (utils.plans_in_collision,
utils.grasp_collision_counts) next to the per-plan host path they replace (utils.plan_in_collision once per plan,
utils.grasp_collision_ratio), on identical inputs: Panda-5k against a 480 x 640 depth observation, T = 50,
B in {1, 64, 853}; 64 grasps x the robot's surface points; Panda-1200 against the sampled shelf (cloud observation) at
B = 64.  Counts are compared before anything is timed.  Median of five timed regions after one warm-up region; a region
ends with the device synchronised (every call is a host-pointer call).  --one B: only one plans_in_collision call at that
B after a warm-up call (for a kernel trace).
    python tools/collision_check_rate.py [--commit TEXT] [--one B]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402  (lib_sha16)
import cloud_sdf_ref as ref  # noqa: E402
import grasptrajopt_amd as g  # noqa: E402
from grasptrajopt_amd import surface_point_cloud as spc  # noqa: E402
from grasptrajopt_amd.utils import grasp_collision_counts, grasp_collision_ratio, plan_in_collision, plans_in_collision  # noqa: E402
from grasptrajopt_amd.synthetic import grasp_poses, random_plans, start_pose, wall_scene  # noqa: E402


def robot_model(name):
    with open(os.path.join(ROOT, "grasptrajopt_amd", "data", f"{name.split('_')[0]}_cfg.json")) as fh:
        cfg = json.load(fh)
    return g.GTORobotModel(desc=g.load_builtin(name), time_derivs=[0, 1], param_joints=cfg["param_joints"],
                           collision_link_names=cfg["collision_link_names"], device=0), cfg


ap = argparse.ArgumentParser()
ap.add_argument("--commit", default="unknown")
ap.add_argument("--one", type=int, default=0)
a = ap.parse_args()


def timed(fn, n=5):
    fn()  # warm-up
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def row(label, new, old):
    r = old[0] / new[0]
    print(f"{label:<58s} new {new[0]:9.3f} ms [{new[1]:.3f} .. {new[2]:.3f}]   per-plan host path {old[0]:10.3f} ms [{old[1]:.3f} .. {old[2]:.3f}]   x{r:.1f}")


depth, K, cam, mask = wall_scene()
dpc = g.DepthPointCloud(depth, K, cam, target_mask=mask, threshold=1.5)
robot, cfg = robot_model("panda_5k")
base = np.array([0.05, -0.03, 0.02])
obs = dpc.observation()
if a.one:
    plans = random_plans(robot.desc, cfg, a.one, seed=1)
    plans_in_collision(robot, obs, plans, base)
    plans_in_collision(robot, obs, plans, base)
    sys.exit(0)

print(f"# tools/collision_check_rate.py on one MI355X; commit {a.commit}, lib_sha16 {bench.lib_sha16()}")
print("# ms per region, median of 5 [min .. max] after one warm-up; new: one plans_in_collision / grasp_collision_counts call against the")
print("# resident observation; per-plan host path: plan_in_collision per plan (gto_eval_points + gto_depth_sdf_cost) / grasp_collision_ratio")
for B in (1, 64, 853):
    plans = random_plans(robot.desc, cfg, B, seed=B)
    new = plans_in_collision(robot, obs, plans, base)[2]
    old = np.stack([plan_in_collision(robot, dpc, p, base)[2] for p in plans])
    assert np.array_equal(new, old), "counts differ"
    row(f"depth 480x640, Panda-5k ({robot.desc.n_points} points), T 50, B {B:4d}",
        timed(lambda: plans_in_collision(robot, obs, plans, base)),
        timed(lambda: [plan_in_collision(robot, dpc, p, base) for p in plans], n=5 if B < 853 else 3))
    print(f"    counts equal: True; plans colliding {int((new > 5).any(axis=1).sum())} of {B}")
print("# waypoints per workgroup of k_check_plans (GTO_CHECK_TG), the same call:")
for B in (64, 853):
    plans = random_plans(robot.desc, cfg, B, seed=B)
    line = []
    for tg in (1, 2, 4):
        os.environ["GTO_CHECK_TG"] = str(tg)
        m = timed(lambda: plans_in_collision(robot, obs, plans, base))
        line.append(f"tg {tg}: {m[0]:.3f} ms [{m[1]:.3f} .. {m[2]:.3f}]")
    del os.environ["GTO_CHECK_TG"]
    print(f"    B {B:4d}   " + "   ".join(line))
qc = start_pose(robot.desc, cfg)
RT = grasp_poses(64, 3)
cnt, P = grasp_collision_counts(robot, obs, RT, qc)
assert np.array_equal(cnt / P, grasp_collision_ratio(robot, dpc, RT, qc)), "ratios differ"
row(f"depth 480x640, 64 grasps x {P} points", timed(lambda: grasp_collision_counts(robot, obs, RT, qc)),
    timed(lambda: grasp_collision_ratio(robot, dpc, RT, qc)))
print(f"    counts equal: True; grasps rejected {int((cnt / P > 0.01).sum())} of 64")
robot.close()

z = np.load(os.path.join(ROOT, "tests", "golden", "surface_cloud.npz"))
pose = np.array([[-1.0, 0, 0, 0.85], [0, -1.0, 0, 0.0], [0, 0, 1.0, -0.1], [0, 0, 0, 1.0]])
parts = [(m, T) for _, m, T in spc.urdf_visual_meshes(ref.shelf_urdf_text(z["shelf_names"], z["shelf_box_size"], z["shelf_box_xyz"]), pose)]
crate = np.eye(4)
crate[:3, 3] = [0.5, 0.0, 0.45]
parts.append((spc.box_mesh([0.25, 0.5, 0.3]), crate))
pts, nrm = spc.place_meshes(parts, samples_per_m2=2.0e4, seed=3)
shelf = g.SurfacePointCloud(pts, nrm)
robot, cfg = robot_model("panda")
plans = random_plans(robot.desc, cfg, 64, seed=64, reach=1.5)
sobs = shelf.observation()
new = plans_in_collision(robot, sobs, plans, base)[2]
old = np.stack([plan_in_collision(robot, shelf, p, base)[2] for p in plans])
assert np.array_equal(new, old), "counts differ"
row(f"cloud {len(pts)} samples k 11, Panda ({robot.desc.n_points} points), T 50, B   64", timed(lambda: plans_in_collision(robot, sobs, plans, base)),
    timed(lambda: [plan_in_collision(robot, shelf, p, base) for p in plans]))
print(f"    counts equal: True; plans colliding {int((new > 5).any(axis=1).sum())} of 64")
robot.close()
