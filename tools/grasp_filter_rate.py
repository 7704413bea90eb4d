#!/usr/bin/env python3
"""grasp_filter_rate.py — time of the grasp collision filter stage of the reference's driver (examples/pybullet_gto_planning.py:
203-236, its `checking_time`), host-composed against stream-ordered, on identical inputs in one process on one MI355X: 64
candidate grasps per object, about 2 000 gripper points, a 480 x 640 depth observation, 1 / 8 / 64 objects.

    host        per object: RT_obj @ RT_g in numpy, utils.grasp_collision_counts (one gto_observation_check_posed round trip),
                ratio test, base subtraction, standoff product and removal of the rejected rows in numpy
    filter      one gto_filter_grasps_device call over all objects with resident inputs, then one synchronisation
    objects     GraspChain.plan_objects on the host path's goal sets (the chain without the stage)
    grasps      GraspChain.plan_grasps (the chain with the stage on the stream)

The kept rows of the two filter paths are compared before anything is timed.  Median of five timed regions after one warm-up
region, the paths alternating; a region ends with the device synchronised.
    python tools/grasp_filter_rate.py [--commit TEXT] [--objects 1,8,64] [--out FILE]
    python tools/grasp_filter_rate.py --host-only --tree DIR   the host row alone with the package of another checkout (one
                                                                from before the entry point: the parent commit's own figure)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--commit", default="unknown")
ap.add_argument("--objects", default="1,8,64")
ap.add_argument("--grasps", type=int, default=64)
ap.add_argument("--points", type=int, default=2000)
ap.add_argument("--out", default=None)
ap.add_argument("--host-only", action="store_true")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
a = ap.parse_args()

ROOT = os.path.abspath(a.tree)
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (lib_sha16)
import grasptrajopt_amd as g  # noqa: E402
from grasptrajopt_amd import synthetic as syn  # noqa: E402
from grasptrajopt_amd import utils  # noqa: E402
from grasptrajopt_amd.grasp_chain import GraspChain  # noqa: E402
import torch  # noqa: E402

with open(os.path.join(ROOT, "grasptrajopt_amd", "data", "panda_cfg.json")) as fh:
    cfg = json.load(fh)
robot = g.GTORobotModel(desc=g.load_builtin("panda_5k"), time_derivs=[0, 1], param_joints=cfg["param_joints"],
                        collision_link_names=cfg["collision_link_names"], device=0)
rng = np.random.default_rng(0)
robot.setup_points_field(rng.uniform([-0.2, -0.6, -0.2], [1.0, 0.6, 0.9], size=(2000, 3)))
wp = robot.workspace_points
qd = np.abs(wp - np.array([0.55, 0.1, 0.1])) - np.array([0.06, 0.06, 0.1])
d_box = np.linalg.norm(np.maximum(qd, 0), axis=1) + np.minimum(qd.max(axis=1), 0)
d_table = wp[:, 2] + 0.1
c_all = syn.sdf_cost_map(np.minimum(d_table, d_box), epsilon=0.06).astype(np.float32)
c_obs = syn.sdf_cost_map(d_table, epsilon=0.06).astype(np.float32)
depth, K, cam, mask = syn.wall_scene()  # 480 x 640
dpc = g.DepthPointCloud(depth, K, cam, target_mask=mask, threshold=1.5)
obs = dpc.observation()
n, P = a.grasps, a.points
pts = rng.uniform([-0.04, -0.1, -0.02], [0.04, 0.1, 0.1], (P, 3))  # a gripper-sized box of surface points
Sc = syn.standoff_pose(-0.03, cfg["axis_standoff"])
Si = syn.standoff_pose(-0.1, cfg["axis_standoff"])
qc = np.array(cfg["default_pose"], dtype=np.float64)
base = np.array([0.01, -0.02, 0.0])
chain = GraspChain(robot, cfg["link_ee"], cfg["link_gripper"], standoff_distance=-0.1, standoff_offset=-10)
chain.bind_scene(5, c_all, c_obs)
h = chain._handle


class Gripper:  # what utils.grasp_collision_counts asks of a gripper model
    def compute_fk_surface_points(self, q):
        return pts, None


def host_stage(O, R):
    """The driver's stage, object by object: counts through one round trip each, the rest in numpy."""
    B = len(O)
    ik_goals, plan_goals, n_out, kept = np.zeros((B, n, 4, 4)), np.zeros((B, n, 4, 4)), np.ones(B, np.int32), []
    for b in range(B):
        RT = O[b] @ R[b]
        counts, Pn = utils.grasp_collision_counts(Gripper(), obs, RT, None, Sc)
        rows = np.flatnonzero(~(counts / Pn > 0.01))
        kept.append(rows)
        take = rows if len(rows) else np.array([0])
        A = RT[take].copy()
        A[:, :3, 3] -= base
        plan_goals[b, :len(take)], ik_goals[b, :len(take)], n_out[b] = A, A @ Si, len(take)
    return ik_goals, plan_goals, n_out, kept


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


cell = lambda t: f"{t[0]:9.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]"
lines = [f"# tools/grasp_filter_rate.py on one MI355X; commit {a.commit}, lib_sha16 {bench.lib_sha16()}",
         f"# {n} grasps per object, {P} gripper points, depth observation {depth.shape[0]} x {depth.shape[1]}, max_ratio 0.01",
         "# ms per region, median of 5 [min .. max] after one warm-up, paths alternating; a region ends synchronised",
         "# host: per object numpy products + utils.grasp_collision_counts + numpy compaction; filter: one gto_filter_grasps_device call",
         "# objects / grasps: GraspChain.plan_objects on the host stage's goal sets / GraspChain.plan_grasps (Panda-5k, T 50, caps 100 / 50)"]
for B in [int(x) for x in a.objects.split(",")]:
    RT, _ = syn.make_goals(robot.desc, robot._util_handle().eval_fk, cfg["link_ee"], B * n, seed=100 + B, zlim=(0.15, 0.6))
    RT = RT.reshape(B, n, 4, 4)
    O = np.tile(np.eye(4), (B, 1, 1))
    O[:, :3, 3] = RT[:, :, :3, 3].mean(axis=1)
    R = np.linalg.inv(O)[:, None] @ RT
    ng = np.full(B, n, np.int32)
    if a.host_only:
        t = timed([lambda: host_stage(O, R)])
        lines.append(f"objects {B:3d}   host {cell(t[0])}   kept {sum(len(k) for k in host_stage(O, R)[3])} of {B * n}")
        print(lines[-1], flush=True)
        continue
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    d_pts, d_O, d_R, d_n, d_base = dev(pts), dev(O), dev(R), dev(ng), dev(np.tile(base, (B, 1)))
    d_cnt, d_keep = torch.empty((B, n), dtype=torch.int32, device="cuda:0"), torch.empty((B, n), dtype=torch.uint8, device="cuda:0")
    d_rows, d_nk, d_ng = (torch.empty(s, dtype=torch.int32, device="cuda:0") for s in ((B, n), (B,), (B,)))
    d_pg, d_ig = (torch.empty((B, n, 16), dtype=torch.float64, device="cuda:0") for _ in range(2))

    def filter_stage():
        h.filter_grasps_device([obs] * B, n, d_pts.data_ptr(), P, d_O.data_ptr(), d_R.data_ptr(), d_n.data_ptr(), Sc, Si, None,
                               d_base.data_ptr(), 0.01, d_cnt.data_ptr(), d_keep.data_ptr(), d_rows.data_ptr(), d_nk.data_ptr(),
                               d_ng.data_ptr(), d_pg.data_ptr(), d_ig.data_ptr(), chain.stream.cuda_stream)
        chain.stream.synchronize()

    kw = dict(axis_standoff=cfg["axis_standoff"])
    ikg, pg, n_out, kept = host_stage(O, R)
    filter_stage()
    nk = d_nk.cpu().numpy()
    same = all(nk[b] == len(kept[b]) and np.array_equal(d_rows[b, :nk[b]].cpu().numpy(), kept[b]) for b in range(B))
    assert nk.sum() > 0, "no grasp was kept: nothing to time"  # (numpy's @ may round a pose differently: `same` is reported)
    t = timed([lambda: host_stage(O, R), filter_stage,
               lambda: chain.plan_objects(qc, ikg, pg, n_out, 5, base, **kw),
               lambda: chain.plan_grasps(qc, O, R, ng, obs, 5, base, pts, Sc, ik_offset=Si, **kw)])
    lines.append(f"objects {B:3d}   host {cell(t[0])}   filter {cell(t[1])}   host/filter x{t[0][0] / t[1][0]:.2f}   "
                 f"plan_objects {cell(t[2])}   plan_grasps {cell(t[3])}   added {t[3][0] - t[2][0]:+.3f} ms")
    lines.append(f"    kept rows equal: {same}; kept {int(nk.sum())} of {B * n}; objects without a kept grasp {int((nk == 0).sum())}")
    print("\n".join(lines[-2:]), flush=True)
text = "\n".join(lines) + "\n"
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
chain.close()
robot.close()
