#!/usr/bin/env python3
"""base_chain_rate.py — the stream-ordered base placement loop against the path it replaces, on the Fetch descriptor.
  (a) GTORobotModel.setup_occupancy_grid from a 480 x 640 depth cloud: the numpy pass on the downloaded points (download
      included: that is what the driver pays) against the device build from the cloud's resident observation;
  (b) 1 / 8 / 64 draws of 10 goals: a loop of BasePlanner.plan_goalset (one solve, one report on the host and one occupancy
      statistic per draw) against BasePlanner.place_base on the same indices.
Results are compared first; then medians of five timed regions with the two paths alternating.
Usage: python tools/base_chain_rate.py [--out profiles/base_chain_rate.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fns, regions=5):
    """Median wall time in ms of each of the callables, run in turn `regions` times (after one untimed turn)."""
    for f in fns:
        f()
    t = [[] for _ in fns]
    for _ in range(regions):
        for k, f in enumerate(fns):
            t0 = time.perf_counter()
            f()
            t[k].append(1e3 * (time.perf_counter() - t0))
    return [float(np.median(x)) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "base_chain_rate.txt"))
    args = ap.parse_args()
    import json
    import torch
    import grasptrajopt_amd as g
    from grasptrajopt_amd import synthetic as syn

    lines = []

    def say(s):
        print(s)
        lines.append(s)

    cfg = json.load(open(os.path.join(ROOT, "grasptrajopt_amd", "data", "fetch_cfg.json")))
    robot = g.GTORobotModel(desc=g.load_builtin("fetch"), time_derivs=[0, 1], param_joints=cfg["param_joints"],
                            collision_link_names=cfg["collision_link_names"], device=0)
    say(f"base_chain_rate: {torch.cuda.get_device_name(0)}, Fetch ({robot.desc.n_points} surface points), medians of 5 regions, paths alternating")

    # ---- (a) the occupancy grid of a 480 x 640 depth image: a wall two metres in front of the robot
    depth, K, cam, _ = syn.wall_scene(480, 640, cam_xyz=(0.6, 0.0, 0.5))

    def grid_numpy():
        dpc = g.DepthPointCloud(depth, K, cam)
        robot.setup_occupancy_grid(np.asarray(dpc.points))  # the cloud comes to the host, then the numpy scatter

    def grid_device():
        dpc = g.DepthPointCloud(depth, K, cam)
        robot.setup_occupancy_grid(dpc.points)  # observation + grid on the device, the grid's bytes come back

    grid_numpy()
    want = {a: getattr(robot, a) for a in ("occupancy_grid", "occupancy_grid_origin", "occupancy_grid_shape", "xgrid", "ygrid")}
    grid_device()
    same = all(np.array_equal(getattr(robot, a), v) for a, v in want.items())
    say(f"(a) grid {robot.occupancy_grid_shape}, {int(robot.occupancy_grid.sum())} occupied nodes; device grid equals numpy grid: {same}")
    if not same:
        raise SystemExit("the two grids differ")
    t_np, t_dev = median_ms([grid_numpy, grid_device])
    say(f"(a) setup_occupancy_grid, 480 x 640 depth cloud: numpy path {t_np:8.2f} ms   device path {t_dev:8.2f} ms   ({t_np / t_dev:.2f}x)")
    occ = robot.occupancy

    # ---- (b) draws of 10 goals: 5 objects, 2 grasps each per draw
    qc = np.array(cfg["default_pose"], dtype=np.float64)
    bp = g.BasePlanner(robot, cfg["link_ee"], cfg["link_gripper"])
    bp.setup_optimization(10, 0.01)
    h = bp._handle
    objs, _ = syn.make_base_goal_sets(robot.desc, h.eval_fk, cfg["link_ee"], qc, 5, 8, seed=0)
    for draws in (1, 8, 64):
        idx = np.random.default_rng(draws).integers(0, 8, (draws, 5, 2))
        sets, _ = bp.draw_goal_sets(objs, indices=idx)

        def loop():
            out = []
            for d in range(draws):  # the parent's path: the driver's loop, run to the end so that both paths do the same work
                out.append(bp.plan_goalset(qc, sets[d]))
            return out

        def chain():
            return bp.place_base(qc, objs, indices=idx, occupancy=occ)

        ref_out, res = loop(), chain()
        cost = np.array([o[4] for o in ref_out])
        first = int(np.flatnonzero(cost == 0)[0]) if (cost == 0).any() else -1
        # the two paths place the footprint by different formulas (an inverse matrix on the host): a point within round-off of
        # a cell edge may fall into another cell, so a count may differ by a point or two; that is reported, not fatal
        diff = np.abs(res.collision - cost.astype(np.int32))
        ok = (res.draw == first and np.array_equal(res.y, ref_out[max(first, 0)][1]) and np.array_equal(res.plan, ref_out[max(first, 0)][0]))
        say(f"(b) {draws:3d} draws: costs {cost.astype(int).tolist()[:8]}{'...' if draws > 8 else ''} first free {first}; place_base agrees: {ok}"
            f" (counts differ at {int((diff > 0).sum())} draws, by at most {int(diff.max())})")
        if not ok or diff.max() > 2:
            raise SystemExit("place_base and the plan_goalset loop differ")
        t_loop, t_chain = median_ms([loop, chain])
        say(f"(b) {draws:3d} draws of 10 goals: plan_goalset loop {t_loop:8.2f} ms   place_base {t_chain:8.2f} ms   ({t_loop / t_chain:.2f}x)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    robot.close()


if __name__ == "__main__":
    main()
