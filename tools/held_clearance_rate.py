#!/usr/bin/env python3
"""held_clearance_rate.py — gto_held_clearance_device on paths of T = 50 columns: Panda (1200 points) and panda_5k, B = 64 and
2048 paths, a cracker box of 256 surface samples in the hand, cutoff inf, 2 x clearance and clearance, against the planners'
default links; gto_self_clearance_device (default mask, cutoff 2 x clearance) and gto_check_held_paths_device (a depth
observation) on the same paths and points as the yardsticks a reader knows.  Every call is warmed up, then timed in five
alternating regions (device events on the stream of the launches); the median and the spread (min .. max) of the five are
reported.

Beside the times, from a HOST-side recount in numpy (no counter in the kernel): the share of (held point, enabled chunk)
pairs whose sphere gap is below the bound the walk STARTS with (the cutoff, or pass A's upper bound) and below the ANSWER
(the least any order of the walk must keep), over RECOUNT_PATHS paths.  The kernel compares a chunk exactly for a whole
wave of 64 held points as soon as one of them survives, so the share of (wave, chunk) items with a survivor is given too.
Usage: python tools/held_clearance_rate.py"""
import copy
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
from self_clearance_rate import chunk_table  # noqa: E402

T, REGIONS, RECOUNT_PATHS, N_BOX = 50, 5, 4, 256
BOX_SIZE, BOX_CENTRE = np.array([0.21, 0.06, 0.16]), np.array([0.0, 0.0, 0.10])  # in panda_hand's frame


def box():
    """N_BOX surface samples of the box in link_ee's frame: faces by area, uniform on the face."""
    rng = np.random.default_rng(3)
    sx, sy, sz = BOX_SIZE
    areas = np.array([sy * sz, sy * sz, sx * sz, sx * sz, sx * sy, sx * sy])
    face = rng.choice(6, size=N_BOX, p=areas / areas.sum())
    u = rng.uniform(-0.5, 0.5, (N_BOX, 3))
    u[np.arange(N_BOX), face // 2] = np.where(face % 2 == 0, -0.5, 0.5)
    return u * BOX_SIZE + BOX_CENTRE


def recount(desc, links, paths, E, local, d2, cutoff):
    """Shares of the (held point, enabled chunk) pairs that survive the sphere test against the starting bound and against
    the answer, the same for (wave of 64 held points, chunk) items, and the enabled chunks."""
    link, centre, radius = chunk_table(desc)
    cd = copy.copy(desc)
    cd.points, cd.point_link = centre, link.astype(np.int32)
    en = links[link]
    start = end = total = w_start = w_end = w_total = 0
    for b in range(paths.shape[0]):
        for t in range(paths.shape[2]):
            c = cd.world_points(paths[b, :, t])[en]
            Y = local @ E[b, t, :3, :3].T + E[b, t, :3, 3]
            D = np.sqrt(((Y[:, None, :] - c[None, :, :]) ** 2).sum(-1))
            gap = np.maximum(D - radius[en][None, :], 0.0)
            bound0 = min(cutoff, float((D + radius[en][None, :]).min()))
            s0, s1 = gap < bound0, gap < min(bound0, np.sqrt(d2[b, t]))
            start, end, total = start + int(s0.sum()), end + int(s1.sum()), total + gap.size
            w_start += sum(int(s0[i:i + 64].any(axis=0).sum()) for i in range(0, len(Y), 64))
            w_end += sum(int(s1[i:i + 64].any(axis=0).sum()) for i in range(0, len(Y), 64))
            w_total += -(-len(Y) // 64) * gap.shape[1]
    return [start / total, end / total], [w_start / w_total, w_end / w_total], int(en.sum())


def run(robot, B):
    desc = load_builtin(robot)
    cfg = json.load(open(os.path.join(ROOT, "grasptrajopt_amd", "data", robot.replace("_5k", "") + "_cfg.json")))
    h = _capi.SolverHandle(desc, cfg["link_ee"], cfg["link_gripper"], _capi.default_opts(), device=0)
    clearance = desc.point_spacing()
    links = desc.held_links(cfg["link_ee"])
    h.set_self_pairs(desc.self_pairs(q_ref=cfg["default_pose"], clearance=clearance))
    rng = np.random.default_rng(5)
    qa, qb = rng.uniform(desc.lower, desc.upper, (2, B, desc.ndof))
    s = np.linspace(0.0, 1.0, T)
    paths = np.ascontiguousarray(qa[:, :, None] * (1 - s) + qb[:, :, None] * s)  # straight lines between two in-limit poses
    fe = desc.frame_index(cfg["link_ee"])
    local = box()
    E_a = h.eval_fk(paths[:, :, 0])[:, fe]  # the box is grasped at every path's first column
    held = np.ascontiguousarray(np.einsum("bij,pj->bpi", E_a[:, :3, :3], local) + E_a[:, None, :3, 3])
    depth, Kc, cam, m = syn.wall_scene()
    obs = g.DepthPointCloud(depth, Kc, cam, target_mask=m, threshold=1.5).observation()
    st = torch.cuda.Stream()
    d_paths, d_held = torch.from_numpy(paths).cuda(), torch.from_numpy(held).cuda()
    d_n = torch.full((B,), N_BOX, dtype=torch.int32, device="cuda")
    d_d2 = torch.empty((B, T), dtype=torch.float64, device="cuda")
    d_link, d_point = (torch.empty((B, T), dtype=torch.int32, device="cuda") for _ in range(2))
    d_pair = torch.empty((B, T, 2), dtype=torch.int32, device="cuda")
    d_sd2, d_cnt = torch.empty((B, T), dtype=torch.float64, device="cuda"), torch.empty((B, T), dtype=torch.int32, device="cuda")
    calls = {"check_held_paths": lambda: h.check_held_paths_device(obs, B, T, d_paths.data_ptr(), d_held.data_ptr(), N_BOX, d_n.data_ptr(),
                                                                   d_cnt.data_ptr(), stream=st.cuda_stream),
             "self_2c": lambda: h.self_clearance_device(B, T, d_paths.data_ptr(), d_sd2.data_ptr(), d_pair.data_ptr(), cutoff=2 * clearance,
                                                        stream=st.cuda_stream)}
    cutoffs = {"inf": np.inf, "2c": 2 * clearance, "c": clearance}
    for name, c in cutoffs.items():
        calls["held_" + name] = (lambda c=c: h.held_clearance_device(B, T, d_paths.data_ptr(), d_held.data_ptr(), N_BOX, d_n.data_ptr(),
                                                                     d_d2.data_ptr(), d_link.data_ptr(), d_point.data_ptr(), links=links,
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
    calls["held_inf"]()
    torch.cuda.synchronize()
    d2 = d_d2.cpu().numpy()
    out = dict(robot=robot, points=desc.n_points, B=B, T=T, held_points=N_BOX, clearance=round(clearance, 5), enabled_links=int(links.sum()),
               columns_below_clearance=int((np.sqrt(d2) < clearance).sum()))
    for name, v in times.items():
        v = sorted(v)
        out[name + "_ms"] = round(v[len(v) // 2], 4)
        out[name + "_ms_min_max"] = [round(v[0], 4), round(v[-1], 4)]
    E = h.eval_fk(paths[:RECOUNT_PATHS].transpose(0, 2, 1).reshape(-1, desc.ndof))[:, fe].reshape(RECOUNT_PATHS, T, 4, 4)
    for name, c in cutoffs.items():
        pairs, items, n_chunks = recount(desc, links, paths[:RECOUNT_PATHS], E, local, d2, c)
        out["survive_" + name] = [round(x, 4) for x in pairs]       # [against the starting bound, against the answer]
        out["survive_waves_" + name] = [round(x, 4) for x in items]
        out["enabled_chunks"] = n_chunks
    h.close()
    return out


if __name__ == "__main__":
    for robot in ("panda", "panda_5k"):
        for B in (64, 2048):
            print(json.dumps(run(robot, B)), flush=True)
