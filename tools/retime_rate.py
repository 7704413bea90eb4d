#!/usr/bin/env python3
"""retime_rate.py — throughput of the batched retiming (gto_retime_batch_device) on device-resident plans: Panda T = 50 at
B = 64, 2048, 16384 and mobile Fetch T = 80 at B = 2048, default limits (URDF velocity, 0.5 rad/s^2), subdiv 2, 100 samples.
The numpy restatement (tests/retime_ref.py) on the host is timed on a few plans for scale.
--paths: the retrieve paths of Panda plans (the 11 columns of a 10-step lift, the 19 of the reversed stretch) at B = 64 and
2048, retimed by gto_retime_paths_device on the planning handle (T = 50) and, for comparison, by gto_retime_batch_device
on a second handle created with T = the path's column count: five alternating regions each, median and min - max.
Usage: python tools/retime_rate.py [--paths]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from grasptrajopt_amd import _capi  # noqa: E402
from grasptrajopt_amd.robot_desc import load_builtin  # noqa: E402
import retime_ref  # noqa: E402


def plans_for(desc, B, T, seed=0):
    rng = np.random.default_rng(seed)
    lo, hi = np.maximum(desc.lower, -3.0), np.minimum(desc.upper, 3.0)
    s = np.linspace(0.0, 1.0, T)
    a = lo + (hi - lo) * rng.uniform(0.2, 0.8, (B, desc.ndof))
    b = lo + (hi - lo) * rng.uniform(0.2, 0.8, (B, desc.ndof))
    P = a[..., None] + (b - a)[..., None] * (3 * s ** 2 - 2 * s ** 3)
    P += 0.05 * np.sin(2 * np.pi * rng.uniform(0.5, 2.0, (B, desc.ndof, 1)) * s + rng.uniform(0, 6, (B, desc.ndof, 1)))
    P[:, desc.param_index] = P[:, desc.param_index, :1]
    return P


def run(name, T, B, reps=20):
    desc = load_builtin(name)
    cfg = json.load(open(os.path.join(ROOT, "grasptrajopt_amd", "data", name.replace("_mobile", "") + "_cfg.json")))
    o = _capi.default_opts()
    o.T = T
    h = _capi.SolverHandle(desc, cfg["link_ee"], cfg["link_gripper"], o, device=0)
    P = plans_for(desc, B, T)
    vm, am = desc.velocity, np.full(desc.ndof, 0.5)
    N, M = 2 * (T - 1) + 1, 100
    Pd = torch.from_numpy(P).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    outs = [torch.empty(B, **f64), torch.empty((B, N), **f64), torch.empty((B, N), **f64), torch.empty((B, M, desc.ndof), **f64),
            torch.empty((B, M, desc.ndof), **f64), torch.empty((B, M, desc.ndof), **f64),
            torch.empty(B, dtype=torch.int32, device="cuda")]
    st = torch.cuda.Stream()  # a stream of its own: the events and the launches are on it
    call = lambda: h.retime_batch_device(B, Pd.data_ptr(), vm, am, 2, M, *(t.data_ptr() for t in outs), stream=st.cuda_stream)
    torch.cuda.synchronize()
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        call()
    e1.record(st)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    not_ok = int((outs[6] != 0).sum())
    nh = 4
    t0 = time.perf_counter()
    retime_ref.retime(P[:nh], vm, am, 2, M)
    host = (time.perf_counter() - t0) / nh
    h.close()
    return dict(robot=name, T=T, B=B, ms=round(ms, 4), plans_per_s=round(B / ms * 1e3), numpy_plans_per_s=round(1 / host, 1),
                status_not_ok=not_ok)


def retrieve_paths(h, desc, B, kind):
    """The retrieve paths of B random plans: "lift" (B, ndof, 11), "reverse" (B, ndof, 19); fingers closed."""
    from grasptrajopt_amd.grasp_chain import finger_joints
    P = plans_for(desc, B, h.T)
    fingers = finger_joints(desc)
    if kind == "lift":
        return h.retrieve_lift(P, 0.3, 10, closed_joints=fingers)["path"]
    path = np.ascontiguousarray(P[:, :, np.arange(-20, -1)][:, :, ::-1])
    path[:, fingers] = 0.0
    return path


def run_paths(B, kind, reps=20, regions=5):
    desc = load_builtin("panda")
    cfg = json.load(open(os.path.join(ROOT, "grasptrajopt_amd", "data", "panda_cfg.json")))
    o = _capi.default_opts()
    o.T = 50
    h = _capi.SolverHandle(desc, cfg["link_ee"], cfg["link_gripper"], o, device=0)
    P = retrieve_paths(h, desc, B, kind)
    Tp = P.shape[2]
    o2 = _capi.default_opts()
    o2.T, o2.standoff_offset = Tp, max(int(o2.standoff_offset), 2 - Tp)  # (a valid standoff waypoint; retiming does not use it)
    h2 = _capi.SolverHandle(desc, cfg["link_ee"], cfg["link_gripper"], o2, device=0)
    vm, am = desc.velocity, np.full(desc.ndof, 0.5)
    N, M = 2 * (Tp - 1) + 1, 100
    Pd = torch.from_numpy(P).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    outs = [torch.empty(B, **f64), torch.empty((B, N), **f64), torch.empty((B, N), **f64), torch.empty((B, M, desc.ndof), **f64),
            torch.empty((B, M, desc.ndof), **f64), torch.empty((B, M, desc.ndof), **f64),
            torch.empty(B, dtype=torch.int32, device="cuda")]
    st = torch.cuda.Stream()
    ptrs = [t.data_ptr() for t in outs]
    calls = dict(paths=lambda: h.retime_paths_device(B, Tp, Pd.data_ptr(), vm, am, None, 2, M, *ptrs, stream=st.cuda_stream),
                 second_handle=lambda: h2.retime_batch_device(B, Pd.data_ptr(), vm, am, 2, M, *ptrs, stream=st.cuda_stream))
    ms = {k: [] for k in calls}
    bits = {}
    for k, call in calls.items():
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        bits[k] = [t.cpu().numpy().tobytes() for t in outs]
    for _ in range(regions):
        for k, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(reps):
                call()
            e1.record(st)
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    not_ok = int((outs[6] != 0).sum())
    h.close()
    h2.close()
    r = dict(robot="panda", kind=kind, Tp=Tp, B=B, same_bits=bits["paths"] == bits["second_handle"], status_not_ok=not_ok)
    for k, v in ms.items():
        r[k + "_ms"] = dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))
    return r


if __name__ == "__main__":
    if "--paths" in sys.argv[1:]:
        for B in (64, 2048):
            for kind in ("lift", "reverse"):
                print(json.dumps(run_paths(B, kind)), flush=True)
        sys.exit(0)
    for name, T, B in (("panda", 50, 64), ("panda", 50, 2048), ("panda", 50, 16384), ("fetch_mobile", 80, 2048)):
        r = run(name, T, B)
        print(json.dumps(r), flush=True)
