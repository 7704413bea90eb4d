#!/usr/bin/env python3
"""held_check_rate.py — what counting the held object's points along the retrieve path costs (gto_check_held_paths_device
inside GraspChain.plan_objects): Panda-5k, a 480 x 640 depth observation with its segmentation image, B = 64 objects of 8
candidate grasps, retrieve = lift (10 steps), retime = None, 1024 held points per object.

    whole call   GraspChain.plan_objects with and without held_points in the retrieve dict, the two alternating; a region is
                 one call and ends synchronised (the chain's one synchronisation).  The call without held_points is the
                 parent's launch for launch.
    stages       the two check stages of that call alone, on the path the call returned, timed with device events on the
                 chain's stream: gto_check_paths_device (the robot's surface points, the existing stage) and
                 gto_check_held_paths_device (the new stage: k_held_attach + k_check_held<true>)

The held counts are compared with a direct host-pointer call, and every other result with the call without held points,
before anything is timed.  Median of five timed regions after one warm-up region.  --one: one call with held points after a
warm-up call (for a kernel trace).
    python tools/held_check_rate.py [--commit TEXT] [--one] [--out FILE]"""
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
ap.add_argument("--one", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()

B, N_GRASPS, P_HELD, STEPS, SOLVE_CAP = 64, 8, 1024, 10, 30
with open(os.path.join(ROOT, "grasptrajopt_amd", "data", "panda_cfg.json")) as fh:
    cfg = json.load(fh)
robot = g.GTORobotModel(desc=g.load_builtin("panda_5k"), time_derivs=[0, 1], param_joints=cfg["param_joints"],
                        collision_link_names=cfg["collision_link_names"], device=0)
rng = np.random.default_rng(0)
robot.setup_points_field(rng.uniform([-0.2, -0.6, -0.2], [1.0, 0.6, 1.0], size=(2000, 3)))
wp = robot.workspace_points
c_obs = syn.sdf_cost_map(wp[:, 2] + 0.1, epsilon=0.06).astype(np.float32)  # a table top 10 cm below the robot's base
chain = GraspChain(robot, cfg["link_ee"], cfg["link_gripper"], standoff_distance=-0.1, standoff_offset=-10)
chain.max_iter = SOLVE_CAP
chain.bind_scene(5, c_obs, c_obs)
depth, K, cam, mask = syn.wall_scene()
obs = g.DepthPointCloud(depth, K, cam, target_mask=mask, threshold=1.5).observation()
labels = np.where(np.asarray(mask) != 0, 1, 0).astype(np.int32)
qc = np.array(cfg["default_pose"], dtype=np.float64)
base = np.zeros(3)
RT, _ = syn.make_goals(robot.desc, robot._util_handle().eval_fk, cfg["link_ee"], B * N_GRASPS, seed=164, zlim=(0.15, 0.6))
RT = RT.reshape(B, N_GRASPS, 4, 4)
held = RT[:, 0, :3, 3][:, None, :] + np.clip(rng.standard_normal((B, P_HELD, 3)) * 0.03, -0.08, 0.08)  # around the first grasp
n_held = np.full(B, P_HELD, np.int32)
lift = dict(mode="lift", distance=0.2, steps=STEPS)
with_held = dict(lift, held_points=held, held_counts=n_held, labels=labels, held_label=1)


def call(retrieve):
    return chain.plan_objects(qc, RT, RT, np.full(B, N_GRASPS, np.int32), 5, base, axis_standoff=cfg["axis_standoff"], observation=obs,
                              retrieve=retrieve, retime=None)


if a.one:
    call(with_held)
    call(with_held)
    sys.exit(0)


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


plain, got = call(lift), call(with_held)
h = chain._handle
same = all(np.ascontiguousarray(v).tobytes() == np.ascontiguousarray(getattr(got, k)).tobytes() for k, v in vars(plain).items())
direct = h.check_held_paths(obs, got.retrieve_path, held, n_held=n_held, labels=labels, held_label=1, base_pos=base)
assert same and np.array_equal(direct, got.retrieve_held_counts), "the call with held points differs from the call without, or from a direct call"
whole = timed([lambda: call(lift), lambda: call(with_held)])

import torch  # noqa: E402
st = chain.stream
cols = STEPS + 1
d_path, d_held, d_n = (torch.from_numpy(np.ascontiguousarray(x)).to(chain.device) for x in (got.retrieve_path, held, n_held))
d_lab, d_hl = torch.from_numpy(labels).to(chain.device), torch.ones(B, dtype=torch.int32, device=chain.device)
d_cnt = torch.empty((B, cols), dtype=torch.int32, device=chain.device)
stages = [lambda: h.check_paths_device(obs, B, cols, d_path.data_ptr(), d_cnt.data_ptr(), base_pos=base, stream=st.cuda_stream),
          lambda: h.check_held_paths_device(obs, B, cols, d_path.data_ptr(), d_held.data_ptr(), P_HELD, d_n.data_ptr(), d_cnt.data_ptr(),
                                            labels=d_lab.data_ptr(), held_label=d_hl.data_ptr(), base_pos=base, stream=st.cuda_stream)]


def region(fn, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


torch.cuda.synchronize()
stage_ms = []
for fn in stages:
    region(fn)  # warm-up
for fn in stages:
    v = sorted(region(fn) for _ in range(5))
    stage_ms.append((v[2], v[0], v[-1]))

fmt = lambda t: f"{t[0]:9.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]"
lines = [f"# tools/held_check_rate.py on one MI355X; commit {a.commit}, lib_sha16 {bench.lib_sha16()}",
         f"# Panda-5k ({robot.desc.n_points} points), depth {depth.shape[0]}x{depth.shape[1]} with labels, B {B} objects x {N_GRASPS} grasps, "
         f"lift of {STEPS} steps ({cols} columns), {P_HELD} held points per object, solve cap {SOLVE_CAP}, retime None",
         "# median of 5 [min .. max] after one warm-up",
         f"every other result equal to the call without held points: {same}; held counts equal to a direct call: True",
         f"held counts: columns with a point inside {int((got.retrieve_held_counts > 0).sum())} of {B * cols}, largest count {int(got.retrieve_held_counts.max())}; "
         f"robot counts: columns with a point inside {int((got.retrieve_counts > 0).sum())} of {B * cols}",
         f"whole call without held_points (the parent's launches)   {fmt(whole[0])}",
         f"whole call with held_points                              {fmt(whole[1])}   difference {whole[1][0] - whole[0][0]:+.3f} ms",
         f"stage gto_check_paths_device ({robot.desc.n_points} points, device events)   {fmt(stage_ms[0])}",
         f"stage gto_check_held_paths_device ({P_HELD} points, device events) {fmt(stage_ms[1])}   x{stage_ms[1][0] / stage_ms[0][0]:.2f} of the existing stage"]
text = "\n".join(lines) + "\n"
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
chain.close()
robot.close()
