#!/usr/bin/env python
"""What solving every goal set from its k best seeds buys: GraspChain.plan_objects(n_seeds=k) on 64 reference-shaped goal
sets of 8 grasps (synthetic.make_goal_sets_reference_shaped) in the Panda table scene of bench.py's reference-shaped figures
(scene seed 0, 128^3 voxels), IK-accepted as the chain does (1 cm, 5 degrees, collision cost < 5).  Per n_seeds in 1, 2, 4, 8:

  class0     share of objects whose chosen plan is in class 0 (valid, reached; no observation is given, so every plan
             counts as free)
  reached    share of objects whose chosen plan ends within 1 cm and 5 degrees of the goal it reached
  ms         one plan_objects call, the median of five after a warm-up call

The row of n_seeds = 1 is slot 0 of the two-seed call for the shares (slot 0 is the one-seed chain bit for bit) and the plain
call, without the argument, for the time.

    python tools/multistart_quality.py [--parent DIR]

--parent DIR: a built checkout of the parent commit; the one-seed call is timed there too, by a child process that imports
the package from DIR (--root DIR --seeds 1), and printed next to this tree's: both make the same launches.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def workload(root):
    sys.path.insert(0, root)
    import grasptrajopt_amd as g
    from grasptrajopt_amd import synthetic as syn
    from grasptrajopt_amd.grasp_chain import GraspChain
    cfg = json.load(open(os.path.join(root, "grasptrajopt_amd", "data", "panda_cfg.json")))
    robot = g.GTORobotModel(desc=g.load_builtin("panda"), time_derivs=[0, 1], param_joints=cfg["param_joints"],
                            collision_link_names=cfg["collision_link_names"], device=0)
    chain = GraspChain(robot, cfg["link_ee"], cfg["link_gripper"])
    h, d = chain._handle, robot.desc
    sc = syn.make_scene(0, n=128, res=2.24 / 128, origin=(-0.4, -1.12, -0.4), table_z=-0.03)
    h.set_scene(0, sc.c_all, sc.c_obs, sc.shape, sc.origin, sc.res)
    moving = d.link_is_moving()[d.point_link]
    qc = np.array(cfg["default_pose"], dtype=np.float64)

    def collision_cost(q):
        return (h.eval_points(0, q, [0.0, 0.0, 0.0], use_obs=True)[2] * moving[None, :]).sum(axis=1)
    RT, _ = syn.make_goal_sets_reference_shaped(d, h.eval_fk, cfg["link_ee"], qc, 64, 8, seed=0, chord_rad=syn.STORED_CHORD_RAD["panda"],
                                                zlim=(0.08, 0.7), collision_cost=collision_cost)
    args = (qc, RT, RT, np.full(64, 8, np.int32), 0, np.zeros(3))
    kw = dict(axis_standoff=cfg["axis_standoff"], pos_tol=0.01, rot_tol_deg=5.0, ik_collision_threshold=5.0)
    return chain, robot, args, kw


def timed(call, repeats=5):
    call()  # warm-up: buffers, LDS limits, the first launch of every kernel
    ms = []
    for _ in range(repeats):
        t = time.perf_counter()
        r = call()
        ms.append(1e3 * (time.perf_counter() - t))
    return r, float(np.median(ms)), ms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--root", default=HERE, help="checkout to import the package from (default: this one)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: time its one-seed call too")
    a = ap.parse_args()
    chain, robot, args, kw = workload(os.path.abspath(a.root))
    rows = {}
    for k in a.seeds:
        if k == 1:
            r, ms, all_ms = timed(lambda: chain.plan_objects(*args, **kw))
            rows[1] = dict(ms=ms, all_ms=all_ms, n_objects=int(len(r.n_accepted)), with_grasp=int((r.n_accepted > 0).sum()))
            continue
        r, ms, all_ms = timed(lambda: chain.plan_objects(*args, n_seeds=k, **kw))
        reached = (r.plan_err_pos < kw["pos_tol"]) & (r.plan_err_rot < kw["rot_tol_deg"])
        rows[k] = dict(class0=float((r.plan_class == 0).mean()), reached=float(reached.mean()), ms=ms, all_ms=all_ms,
                       best_slot_counts=np.bincount(r.best_slot, minlength=k).tolist(), with_grasp=int((r.n_accepted > 0).sum()))
        if 1 in rows and "class0" not in rows[1]:  # slot 0 is the one-seed chain
            r0 = (r.slot_err_pos[:, 0] < kw["pos_tol"]) & (r.slot_err_rot[:, 0] < kw["rot_tol_deg"])
            rows[1].update(class0=float((r.slot_class[:, 0] == 0).mean()), reached=float(r0.mean()))
    chain.close()
    robot.close()
    print(f"{'n_seeds':>8} {'class0':>8} {'reached':>8} {'ms':>9}   (64 objects x 8 grasps, Panda, max_iter 100)")
    for k in sorted(rows):
        v = rows[k]
        print(f"{k:>8} {v.get('class0', float('nan')):>8.3f} {v.get('reached', float('nan')):>8.3f} {v['ms']:>9.2f}   "
              f"calls {[round(x, 2) for x in v['all_ms']]} objects with an accepted grasp {v['with_grasp']}"
              + (f" best_slot counts {v['best_slot_counts']}" if "best_slot_counts" in v else ""))
    if a.parent:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", os.path.abspath(a.parent), "--seeds", "1"],
                             capture_output=True, text=True, timeout=600)
        line = [l for l in out.stdout.splitlines() if l.strip().startswith("1 ")]
        print("parent commit, one seed:", line[0].strip() if line else f"failed ({out.returncode}): {out.stderr[-400:]}")
    print(json.dumps({"multistart_quality": {str(k): {x: y for x, y in v.items() if x != "all_ms"} for k, v in rows.items()}}))


if __name__ == "__main__":
    main()
