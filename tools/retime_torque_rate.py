#!/usr/bin/env python3
"""retime_torque_rate.py — paths per second of the torque-limited retiming (gto_retime_paths_torque_device) next to the
convex one (gto_retime_paths_convex_device) on the same device-resident paths and the same vmax / amax, alternating in one
process: Panda plans of T = 50 at subdiv 2 (N = 99) and the 11 columns of a 10-step lift (N = 21), at B = 64 and 2048; after
a warm-up, five regions of each, median and min - max.  The Panda carries the inertials and effort limits of
tests/golden/panda_inertials.json; the lift carries 1 kg, the approach plans nothing; amax = 50 rad/s^2, so that torque and
velocity decide.  With each workload: the Newton steps per path of both calls (mean, max), the statuses, and how much longer
the torque-limited profile is where both converged.

--trace: one short call of each kind and nothing else, for a kernel trace of the launch list (k_retime_torque_rows and
k_retime_tau beside the solve).
Usage: python tools/retime_torque_rate.py [--trace] [--reps R]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(kind, B, reps, regions=5, trace=False):
    import torch
    import dynamics_ref as dr
    from grasptrajopt_amd import _capi
    from grasptrajopt_amd.robot_desc import load_builtin
    from retime_rate import plans_for, retrieve_paths
    desc = dr.with_fixture_inertials(load_builtin("panda"), "panda")
    cfg = json.load(open(os.path.join(ROOT, "grasptrajopt_amd", "data", "panda_cfg.json")))
    o = _capi.default_opts()
    o.T = 50
    h = _capi.SolverHandle(desc, cfg["link_ee"], cfg["link_gripper"], o, device=0)
    P = plans_for(desc, B, 50) if kind == "plans" else retrieve_paths(h, desc, B, "lift")
    Tp = P.shape[2]
    vm, am = desc.velocity, np.full(desc.ndof, 50.0)
    N, M = 2 * (Tp - 1) + 1, 100
    Pd = torch.from_numpy(np.ascontiguousarray(P)).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    mass = torch.full((B,), 1.0, **f64) if kind == "lift" else None

    def outputs(n_samples):
        return ([torch.empty(B, **f64), torch.empty((B, N), **f64), torch.empty((B, N), **f64)] +
                [torch.empty((B, M, desc.ndof), **f64) for _ in range(n_samples)] +
                [torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")])

    oc, ot = outputs(3), outputs(4)
    st = torch.cuda.Stream()
    pc, pt = [t.data_ptr() for t in oc], [t.data_ptr() for t in ot]
    calls = dict(convex=lambda: h.retime_paths_convex_device(B, Tp, Pd.data_ptr(), vm, am, None, 2, M, 1e-8, _capi.RETIME_MAX_NEWTON,
                                                             *pc, stream=st.cuda_stream),
                 torque=lambda: h.retime_paths_torque_device(B, Tp, Pd.data_ptr(), vm, am, None, None if mass is None else mass.data_ptr(),
                                                             None, None, None, 2, M, 1e-8, _capi.RETIME_MAX_NEWTON, *pt,
                                                             stream=st.cuda_stream))
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
    sc, stq = oc[-2].cpu().numpy(), ot[-2].cpu().numpy()
    dcv, dtq = oc[0].cpu().numpy(), ot[0].cpu().numpy()
    ic, it = oc[-1].cpu().numpy(), ot[-1].cpu().numpy()
    both = (sc == 0) & (stq == 0)
    longer = dtq[both] / dcv[both] - 1.0
    h.close()
    r = dict(workload=kind, Tp=Tp, N=N, B=B, payload_kg=0.0 if mass is None else 1.0,
             torque_status={int(s): int((stq == s).sum()) for s in np.unique(stq)}, convex_not_converged=int((sc != 0).sum()),
             newton_convex=[round(float(ic.mean()), 1), int(ic.max())], newton_torque=[round(float(it[both].mean()), 1), int(it.max())],
             longer_mean=float(np.round(longer.mean(), 4)), longer_max=float(np.round(longer.max(), 4)),
             shorter_max=float(longer.min() < -1e-8 and -longer.min()))
    for k, v in ms.items():
        if v:
            med = float(np.median(v))
            r[k] = dict(ms_median=round(med, 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), paths_per_s=round(B / med * 1e3))
    if ms["torque"]:
        r["torque_over_convex"] = round(float(np.median(ms["torque"]) / np.median(ms["convex"])), 2)
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
