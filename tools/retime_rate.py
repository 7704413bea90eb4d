#!/usr/bin/env python3
"""retime_rate.py — throughput of the batched retiming (gto_retime_batch_device) on device-resident plans: Panda T = 50 at
B = 64, 2048, 16384 and mobile Fetch T = 80 at B = 2048, default limits (URDF velocity, 0.5 rad/s^2), subdiv 2, 100 samples.
The numpy restatement (tests/retime_ref.py) on the host is timed on a few plans for scale.
Usage: python tools/retime_rate.py"""
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


if __name__ == "__main__":
    for name, T, B in (("panda", 50, 64), ("panda", 50, 2048), ("panda", 50, 16384), ("fetch_mobile", 80, 2048)):
        r = run(name, T, B)
        print(json.dumps(r), flush=True)
