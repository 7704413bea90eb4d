#!/usr/bin/env python3
"""inverse_dynamics_rate.py — rows per second of gto_inverse_dynamics (host pointers, synchronous: staging copies, one launch
of k_inverse_dynamics, one synchronisation) on Panda and Fetch with the inertials of tests/golden: n = 67, 6336 (the
gridpoints of 64 plans of T = 50 at subdiv 2) and 202752 (2048 such plans), without and with a payload; after a warm-up,
five regions of `reps` calls each by the host clock, median and min - max per call.

Usage: python tools/inverse_dynamics_rate.py [--reps R]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(name, n, payload, reps, regions=5):
    import dynamics_cases as dc
    import dynamics_ref as dr
    from grasptrajopt_amd import _capi
    desc, ee, gr, _ = dc.robot(name)
    h = _capi.SolverHandle(desc, ee, gr, device=0)
    q, qd, qdd = dr.in_limit_states(desc, n, seed=1)
    pl = {"mass": np.full(n, 2.0), "com": np.tile([0.0, 0.0, 0.1], (n, 1))} if payload else None
    for _ in range(3):
        tau = h.inverse_dynamics(q, qd, qdd, pl)
    ms = []
    for _ in range(regions):
        t0 = time.perf_counter()
        for _ in range(reps):
            h.inverse_dynamics(q, qd, qdd, pl)
        ms.append((time.perf_counter() - t0) / reps * 1e3)
    h.close()
    med = float(np.median(ms))
    return dict(robot=name, n_frames=desc.n_frames, n=n, payload=bool(payload), tau_inf=round(float(np.abs(tau).max()), 3),
                ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), rows_per_s=round(n / med * 1e3))


if __name__ == "__main__":
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 10
    for name in ("panda", "fetch"):
        for n in (67, 6336, 202752):
            for payload in (False, True):
                print(json.dumps(run(name, n, payload, reps)), flush=True)
