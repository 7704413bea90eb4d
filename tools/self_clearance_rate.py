#!/usr/bin/env python3
"""self_clearance_rate.py — gto_self_clearance_device on paths of T = 50 columns: Panda (1200 points) and panda_5k, B = 64 and
2048 paths, cutoff inf, 2 x clearance and clearance, under the planners' default mask; gto_check_paths_device against a depth
observation on the same paths as the yardstick a reader knows.  Every call is warmed up, then timed in five alternating
regions (device events on the stream of the launches); the median and the spread (min .. max) of the five are reported.

Beside the times, from a HOST-side recount in numpy (no counter in the kernel): the share of enabled chunk pairs whose sphere
gap is below the bound the walk STARTS with (the cutoff, or pass A's upper bound: the most the kernel compares exactly) and
below the ANSWER (the least any order of the walk must compare), over RECOUNT_PATHS paths; and for cutoff inf the FP64 rate
those two counts bracket, at 8 flops per point pair (3 differences, 3 products, 2 sums) over 64 x 64 slots per chunk pair,
against PEAK_FP64 (the vector FP64 peak AMD publishes for the MI355X; the kernel issues no matrix-core FP64 in its walk).
The recount restates gto_robot.h's chunk table (Morton order inside a link, runs of 64, mean-centred spheres).
Usage: python tools/self_clearance_rate.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import grasptrajopt_amd as g  # noqa: E402
from grasptrajopt_amd import _capi, synthetic as syn  # noqa: E402
from grasptrajopt_amd.robot_desc import load_builtin  # noqa: E402

T, REGIONS, RECOUNT_PATHS = 50, 5, 4
PEAK_FP64 = 78.6e12  # flop/s


def chunk_table(desc):
    """(link (C,), centre (C, 3) in the link's visual frame, radius (C,)) as gto_robot.h builds them."""
    def spread(v):
        v = v & 0x3ff
        v = (v | (v << 16)) & 0x30000ff
        v = (v | (v << 8)) & 0x300f00f
        v = (v | (v << 4)) & 0x30c30c3
        return (v | (v << 2)) & 0x9249249
    link, centre, radius = [], [], []
    for l in range(desc.n_links):
        x = desc.points[desc.point_link == l]
        if not len(x):
            continue
        lo, ext = x.min(0), max(1e-12, float((x.max(0) - x.min(0)).max()))
        q = np.clip((x - lo) / ext * 1023.0, 0.0, 1023.0).astype(np.uint32)
        code = spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
        x = x[np.argsort(code, kind="stable")]
        for i in range(0, len(x), 64):
            c = x[i:i + 64].mean(0)
            link.append(l), centre.append(c), radius.append(np.sqrt(((x[i:i + 64] - c) ** 2).sum(1).max()))
    return np.array(link), np.array(centre), np.array(radius)


def recount(desc, mask, paths, d2, cutoff):
    """Shares of the enabled chunk pairs that survive the sphere test against the starting bound and against the answer."""
    import copy
    link, centre, radius = chunk_table(desc)
    cd = copy.copy(desc)
    cd.points, cd.point_link = centre, link.astype(np.int32)
    en = np.triu(mask[link][:, link], 1)
    rsum = radius[:, None] + radius[None, :]
    start = end = total = 0
    for b in range(paths.shape[0]):
        for t in range(paths.shape[2]):
            c = cd.world_points(paths[b, :, t])
            D = np.sqrt(((c[:, None, :] - c[None, :, :]) ** 2).sum(-1))
            gap = np.maximum(D - rsum, 0.0)[en]
            bound0 = min(cutoff, float((D + rsum)[en].min()))
            start += int((gap < bound0).sum())
            end += int((gap < min(bound0, np.sqrt(d2[b, t]))).sum())
            total += gap.size
    return start / total, end / total, total / (paths.shape[0] * paths.shape[2])


def run(robot, B):
    desc = load_builtin(robot)
    cfg = json.load(open(os.path.join(ROOT, "grasptrajopt_amd", "data", robot.replace("_5k", "") + "_cfg.json")))
    h = _capi.SolverHandle(desc, cfg["link_ee"], cfg["link_gripper"], _capi.default_opts(), device=0)
    clearance = desc.point_spacing()
    mask = desc.self_pairs(q_ref=cfg["default_pose"], clearance=clearance)
    h.set_self_pairs(mask)
    rng = np.random.default_rng(5)
    qa, qb = rng.uniform(desc.lower, desc.upper, (2, B, desc.ndof))
    s = np.linspace(0.0, 1.0, T)
    paths = np.ascontiguousarray(qa[:, :, None] * (1 - s) + qb[:, :, None] * s)  # straight lines between two in-limit poses
    depth, Kc, cam, m = syn.wall_scene()
    obs = g.DepthPointCloud(depth, Kc, cam, target_mask=m, threshold=1.5).observation()
    st = torch.cuda.Stream()
    d_paths = torch.from_numpy(paths).cuda()
    d_d2 = torch.empty((B, T), dtype=torch.float64, device="cuda")
    d_pair = torch.empty((B, T, 2), dtype=torch.int32, device="cuda")
    d_cnt = torch.empty((B, T), dtype=torch.int32, device="cuda")
    calls = {"check_paths": lambda: h.check_paths_device(obs, B, T, d_paths.data_ptr(), d_cnt.data_ptr(), stream=st.cuda_stream)}
    cutoffs = {"inf": np.inf, "2c": 2 * clearance, "c": clearance}
    for name, c in cutoffs.items():
        calls["self_" + name] = (lambda c=c: h.self_clearance_device(B, T, d_paths.data_ptr(), d_d2.data_ptr(), d_pair.data_ptr(),
                                                                     cutoff=c, stream=st.cuda_stream))

    def region(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    torch.cuda.synchronize()
    reps = {}
    for name, fn in calls.items():
        fn()
        torch.cuda.synchronize()
        reps[name] = max(2, min(200, int(150.0 / max(region(fn, 2), 1e-3))))  # about 0.15 s per region
    times = {name: [] for name in calls}
    for _ in range(REGIONS):
        for name, fn in calls.items():
            times[name].append(region(fn, reps[name]))
    calls["self_inf"]()
    torch.cuda.synchronize()
    d2 = d_d2.cpu().numpy()
    out = dict(robot=robot, points=desc.n_points, B=B, T=T, clearance=round(clearance, 5), enabled_link_pairs=int(mask.sum() // 2),
               columns_below_clearance=int((np.sqrt(d2) < clearance).sum()))
    for name, v in times.items():
        v = sorted(v)
        out[name + "_ms"] = round(v[len(v) // 2], 4)
        out[name + "_ms_min_max"] = [round(v[0], 4), round(v[-1], 4)]
    for name, c in cutoffs.items():
        a, e, per_col = recount(desc, mask, paths[:RECOUNT_PATHS], d2, c)
        out["survive_" + name] = [round(a, 4), round(e, 4)]  # [against the starting bound, against the answer]
        if name == "inf":
            flops = [share * per_col * 64 * 64 * 8 * B * T for share in (a, e)]
            rate = [f / (out["self_inf_ms"] * 1e-3) for f in flops]
            out["chunk_pairs_per_column"] = round(per_col, 1)
            out["fp64_tflops_inf"] = [round(r / 1e12, 3) for r in rate]
            out["fp64_share_of_peak_inf"] = [round(r / PEAK_FP64, 4) for r in rate]
    h.close()
    return out


if __name__ == "__main__":
    for robot in ("panda", "panda_5k"):
        for B in (64, 2048):
            print(json.dumps(run(robot, B)), flush=True)
