#!/usr/bin/env python3
"""track_rollout_rate.py — paths and control periods per second of gto_track_rollout (host pointers, synchronous: staging
copies, one launch of k_track_rollout, one synchronisation) on Panda and Fetch with the inertials of tests/golden, at B = 64
and 2048 paths: a 3 s reference (a raised-cosine move of 0.3 rad, 0.03 m on a prismatic joint, from the default pose, 100
samples) followed at dt = 1 ms, 3000 control periods of one RK4 step each, full feedforward, gains for a natural frequency of
30 rad/s at damping 0.7 on the mass matrix's diagonal, the description's effort limits, 2 kg in the hand that the controller
knows about.  After a warm-up call, five regions of `reps` calls each by the host clock,
median and min - max per call.

Usage: python tools/track_rollout_rate.py [--reps R]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DURATION, DT, M = 3.0, 1e-3, 100


def run(name, B, reps, regions=5):
    import dynamics_cases as dc
    import forward_ref as fr
    from grasptrajopt_amd import _capi
    desc, ee, gr, _ = dc.robot(name)
    with open(os.path.join(ROOT, "grasptrajopt_amd", "data", f"{name}_cfg.json")) as fh:
        pose = np.array(json.load(fh)["default_pose"], dtype=np.float64)
    h = _capi.SolverHandle(desc, ee, gr, device=0)
    free = fr.free_joints(desc)
    prismatic = np.zeros(desc.ndof, dtype=bool)
    for f in range(desc.n_frames):
        if desc.joint_type[f] == 2 and desc.q_index[f] >= 0:
            prismatic[desc.q_index[f]] = True
    rng = np.random.default_rng(1)
    amp = np.where(free, np.where(prismatic, 0.03, 0.3), 0.0) * rng.uniform(-1.0, 1.0, (B, 1, desc.ndof))
    x = np.linspace(0.0, 1.0, M)[None, :, None]
    q = pose + amp * 0.5 * (1 - np.cos(np.pi * x))
    qd = amp * 0.5 * np.pi * np.sin(np.pi * x) / DURATION
    qdd = amp * 0.5 * np.pi ** 2 * np.cos(np.pi * x) / DURATION ** 2
    dur = np.full(B, DURATION)
    pl = {"mass": 2.0, "com": [0.0, 0.0, 0.1]}
    # gains from the mass matrix's diagonal at the default pose: natural frequency 30 rad/s, damping ratio 0.7 per joint (one
    # pair of numbers for every joint makes the zero-order hold unstable on Fetch's wrist, whose inertia is 1e-3 of the shoulder's)
    inertia = np.diagonal(h.forward_dynamics(pose, 0 * pose, 0 * pose, pl, want_mass_matrix=True)[2][0])
    kp, kd = np.where(free, 30.0 ** 2 * inertia, 0.0), np.where(free, 2 * 0.7 * 30.0 * inertia, 0.0)
    kw = dict(dt=DT, n_samples=100, feedforward="full", model_payload=pl, plant_payload=pl)
    out = h.track_rollout(dur, q, qd, qdd, kp, kd, **kw)
    ms = []
    for _ in range(regions):
        t0 = time.perf_counter()
        for _ in range(reps):
            h.track_rollout(dur, q, qd, qdd, kp, kd, **kw)
        ms.append((time.perf_counter() - t0) / reps * 1e3)
    h.close()
    med, steps = float(np.median(ms)), int(out["steps"].sum())
    return dict(robot=name, n_frames=desc.n_frames, free_joints=int(free.sum()), B=B, steps_per_path=int(out["steps"][0]),
                status_ok=int((out["status"] == 0).sum()), err_max=float(f"{np.nanmax(out['err_max']):.3e}"),
                sat_steps_max=int(out["sat_steps"].max()), ms_median=round(med, 2), ms_min=round(min(ms), 2), ms_max=round(max(ms), 2),
                paths_per_s=round(B / med * 1e3, 1), periods_per_s=round(steps / med * 1e3))


if __name__ == "__main__":
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 1
    for name in ("panda", "fetch"):
        for B in (64, 2048):
            print(json.dumps(run(name, B, reps)), flush=True)
