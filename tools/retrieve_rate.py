#!/usr/bin/env python3
"""retrieve_rate.py — the lift after the grasp (gto_retrieve_lift_device: K = 10 IK steps per plan in ONE launch) against the
same chain as K stream-ordered calls of gto_solve_ik_pose_batch_device with the goal of every step written in between (what
a caller could do before the fused entry point existed; RT0 and the first column are prepared outside the timed region, in
its favour).  Panda, B = 64 and 2048 plans, without and with the collision term.  Both routes are warmed up, then timed in
five alternating regions each (device events on the stream of the launches); the median and the spread (min .. max) of the
five are reported, and the two routes' paths are compared bit for bit.
Usage: python tools/retrieve_rate.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from grasptrajopt_amd import _capi, synthetic as syn  # noqa: E402
import retrieve_ref as rr  # noqa: E402

K, DIST, MAX_ITER, REGIONS = 10, 0.2, 50, 5


def run(B, collide):
    desc, cfg, plans = rr.grasp_plans("panda", B, seed=1)
    h = _capi.SolverHandle(desc, cfg["link_ee"], cfg["link_gripper"], _capi.default_opts(), device=0)
    sc = syn.make_scene(3, n=48, res=0.0467)
    h.set_scene(0, sc.c_all, sc.c_obs, sc.shape, sc.origin, sc.res)
    closed = rr.finger_joints(desc)
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    d_plans = torch.from_numpy(plans).cuda()
    d_sid = torch.zeros(B, **i32) if collide else None
    d_base = torch.zeros((B, 3), **f64) if collide else None
    sid_p, base_p = (d_sid.data_ptr(), d_base.data_ptr()) if collide else (None, None)
    # fused
    d_path, d_it, d_stat = torch.empty((B, desc.ndof, K + 1), **f64), torch.empty((B, K), **i32), torch.empty((B, K), **i32)
    d_reached = torch.empty(B, **i32)

    def fused():
        h.retrieve_lift_device(B, d_plans.data_ptr(), sid_p, base_p, (0.0, 0.0, 1.0), DIST, K, closed, 0.0, MAX_ITER, rr.POS_TOL,
                               rr.ROT_TOL_DEG, d_path.data_ptr(), iters_out=d_it.data_ptr(), status_out=d_stat.data_ptr(),
                               reached_out=d_reached.data_ptr(), stream=st.cuda_stream)

    # composed: column 0 and RT0 from the host (not timed), then per step the goal update and one IK launch
    q0 = rr.column0(plans, closed, 0.0)
    RT0 = h.eval_fk(q0)[:, desc.frame_index(cfg["link_ee"])]
    d_RT0, d_goal = torch.from_numpy(np.ascontiguousarray(RT0.reshape(B, 16))).cuda(), torch.empty((B, 16), **f64)
    d_cols = torch.empty((K + 1, B, desc.ndof), **f64)
    d_cols[0].copy_(torch.from_numpy(q0))
    d_cit, d_cstat = torch.empty((K, B), **i32), torch.empty((K, B), **i32)
    step = DIST / K

    def composed():
        with torch.cuda.stream(st):
            for k in range(1, K + 1):
                d_goal.copy_(d_RT0)
                d_goal[:, 11] += k * step  # direction (0, 0, 1): x and y get + 0.0
                h.solve_ik_pose_batch_device(0, B, sid_p, d_cols[k - 1].data_ptr(), d_goal.data_ptr(), base_p, MAX_ITER,
                                             d_cols[k].data_ptr(), None, d_cit[k - 1].data_ptr(), d_cstat[k - 1].data_ptr(), st.cuda_stream)

    torch.cuda.synchronize()
    for _ in range(3):
        fused()
        composed()
    torch.cuda.synchronize()
    same = bool(torch.equal(d_path, d_cols.permute(1, 2, 0))) and bool(torch.equal(d_it, d_cit.t()))
    iters, reached = float(d_it.double().mean()), int((d_reached == K).sum())

    def region(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    reps = max(5, int(300.0 / max(region(composed, 3), 1e-3)))  # about 0.3 s per region of the slower route
    t = {"fused": [], "composed": []}
    for _ in range(REGIONS):
        t["fused"].append(region(fused, reps))
        t["composed"].append(region(composed, reps))
    h.close()
    out = dict(robot="panda", B=B, K=K, collide=collide, reps=reps, same_bits=same, mean_iters_per_step=round(iters, 2), reached_all=reached)
    for name, v in t.items():
        v = sorted(v)
        out[name + "_ms"] = round(v[len(v) // 2], 4)
        out[name + "_ms_min_max"] = [round(v[0], 4), round(v[-1], 4)]
    out["fused_chains_per_s"] = round(B / out["fused_ms"] * 1e3)
    out["speedup"] = round(out["composed_ms"] / out["fused_ms"], 3)
    return out


if __name__ == "__main__":
    for B in (64, 2048):
        for collide in (False, True):
            print(json.dumps(run(B, collide)), flush=True)
