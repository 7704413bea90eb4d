#!/usr/bin/env python3
"""retime_convex_rate.py — plans per second of the convex retiming (gto_retime_paths_convex_device) next to the greedy one
(gto_retime_paths_device) on device-resident paths, alternating in one process: Panda plans of T = 50 at subdiv 2 and the
11 columns of a 10-step lift, at B = 64 and 2048; after a warm-up, five regions of each, median and min - max.  With each
workload: the Newton steps per path (mean, max), the share of paths the greedy pass flags, and how much shorter the optimum
is where both converged.

The library is the one GTO_HIP_LIB names, or the tree's own.  --trace: one short call of each kind and nothing else, for a
kernel trace of the launch list.
Usage: python tools/retime_convex_rate.py [--trace] [--reps R]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

def workload(h, desc, kind, B):
    from retime_rate import plans_for, retrieve_paths
    return plans_for(desc, B, 50) if kind == "plans" else retrieve_paths(h, desc, B, "lift")


def run(kind, B, reps, regions=5, trace=False):
    import torch
    from grasptrajopt_amd import _capi
    from grasptrajopt_amd.robot_desc import load_builtin
    desc = load_builtin("panda")
    cfg = json.load(open(os.path.join(ROOT, "grasptrajopt_amd", "data", "panda_cfg.json")))
    o = _capi.default_opts()
    o.T = 50
    h = _capi.SolverHandle(desc, cfg["link_ee"], cfg["link_gripper"], o, device=0)
    P = workload(h, desc, kind, B)
    Tp = P.shape[2]
    vm, am = desc.velocity, np.full(desc.ndof, 0.5)
    N, M = 2 * (Tp - 1) + 1, 100
    Pd = torch.from_numpy(np.ascontiguousarray(P)).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")

    def outputs():
        return [torch.empty(B, **f64), torch.empty((B, N), **f64), torch.empty((B, N), **f64), torch.empty((B, M, desc.ndof), **f64),
                torch.empty((B, M, desc.ndof), **f64), torch.empty((B, M, desc.ndof), **f64),
                torch.empty(B, dtype=torch.int32, device="cuda")]

    og, oc, iters = outputs(), outputs(), torch.empty(B, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    pg, pc = [t.data_ptr() for t in og], [t.data_ptr() for t in oc]
    calls = dict(greedy=lambda: h.retime_paths_device(B, Tp, Pd.data_ptr(), vm, am, None, 2, M, *pg, stream=st.cuda_stream),
                 convex=lambda: h.retime_paths_convex_device(B, Tp, Pd.data_ptr(), vm, am, None, 2, M, 1e-8, _capi.RETIME_MAX_NEWTON,
                                                             *pc, iters.data_ptr(), stream=st.cuda_stream))
    for call in calls.values():
        for _ in range(1 if trace else 3):
            call()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(0 if trace else regions):
        for k, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(reps):
                call()
            e1.record(st)
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    sg, sc = og[6].cpu().numpy(), oc[6].cpu().numpy()
    dg, dc, it = og[0].cpu().numpy(), oc[0].cpu().numpy(), iters.cpu().numpy()
    both = (sg == 0) & (sc == 0)
    gain = 1.0 - dc[both] / dg[both]
    h.close()
    r = dict(workload=kind, Tp=Tp, N=N, B=B, lib=os.path.basename(os.environ.get("GTO_HIP_LIB", "libgto_hip.so")),
             greedy_flagged_share=round(float((sg != 0).mean()), 4), convex_not_converged=int((sc != 0).sum()),
             newton_mean=round(float(it.mean()), 1), newton_max=int(it.max()),
             shorter_mean=float(np.round(gain.mean(), 5)), shorter_max=float(np.round(gain.max(), 5)),
             longer_max=float(gain.min() < -1e-8 and -gain.min()))
    for k, v in ms.items():
        if v:
            med = float(np.median(v))
            r[k] = dict(ms_median=round(med, 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), plans_per_s=round(B / med * 1e3))
    if ms["convex"]:
        r["convex_over_greedy"] = round(float(np.median(ms["convex"]) / np.median(ms["greedy"])), 1)
    return r


if __name__ == "__main__":
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 10
    if "--trace" in args:
        print(json.dumps(run("lift", 64, 1, trace=True)), flush=True)
        sys.exit(0)
    for kind in ("plans", "lift"):
        for B in (64, 2048):
            print(json.dumps(run(kind, B, reps)), flush=True)
