#!/usr/bin/env python3
"""The launches at the start of a solve call, from a rocprofv3 --kernel-trace CSV: for the calls of B instances (default:
the largest B in the trace) the init pass (the first k_obstacle_gram behind k_lm_init), the kernels around it in front of round 0
(k_init_heads, k_ss_fixed_spread, k_seed_broad by grid) and round 0's obstacle launch: grid (workgroups) and duration, and their
sum as a share of the call's time on its queue (k_lm_init's start .. k_lm_finalize's end) and of all kernel time in the trace.
usage: tools/start_launches.py <kernel_trace.csv> [B]"""
import collections
import csv
import statistics
import sys

rows = []
for r in csv.DictReader(open(sys.argv[1])):
    name = r["Kernel_Name"].replace("void ", "").split("(")[0].split("<")[0]
    wg = int(r.get("Workgroup_Size_X", r.get("Workgroup_Size", 1)) or 1)
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name, r.get("Queue_Id", "?"),
                 int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0) // max(wg, 1)))
rows.sort()
all_kernel_ns = sum(e - s for s, e, *_ in rows)
byq = collections.defaultdict(list)
for row in rows:
    byq[row[3]].append(row)
calls = []
for q, v in byq.items():
    cur = None
    for s, e, n, _, g in v:
        if n == "k_lm_init":
            if cur is None or cur["ev"]:  # (a call with lanes has one k_lm_init per lane, back to back)
                cur = {"t0": s, "B": 0, "ev": []}
            cur["B"] += g
        elif cur is not None and n == "k_lm_finalize":
            cur["t1"] = e
            calls.append(cur)
            cur = None
        elif cur is not None:
            cur["ev"].append((n, g, e - s))
want = int(sys.argv[2]) if len(sys.argv) > 2 else max(c["B"] for c in calls)
calls = [c for c in calls if c["B"] == want]
parts = collections.defaultdict(list)  # label -> [(grid, ns)]
start_ns, wall_ns = [], []
for c in calls:
    ev, tot, n_obs = c["ev"], 0, 0
    for n, g, d in ev:
        if n == "k_obstacle_gram":
            n_obs += 1
            label = "init pass" if n_obs == 1 else "round 0 obstacle"
        elif n_obs <= 1 and n != "k_lm_step":  # k_init_heads in front of the init pass; the spread and the seed tests behind it
            label = f"{n} ({g})" if n == "k_seed_broad" else n
        else:
            label = None
        if label:
            parts[label].append((g, d))
            tot += d
        if n_obs == 2:
            break
    start_ns.append(tot)
    wall_ns.append(c["t1"] - c["t0"])
print(f"{len(calls)} calls of B = {want}; all kernel time in the trace {all_kernel_ns / 1e6:.2f} ms")
for label, v in parts.items():
    d = [x[1] / 1e3 for x in v]
    print(f"  {label:20s} n {len(v):4d}  grid {statistics.median(x[0] for x in v):7.0f}  us median {statistics.median(d):7.1f}  mean {statistics.mean(d):7.1f}  min {min(d):7.1f}  max {max(d):7.1f}")
if calls:
    # (b): these calls' start-up launches against the kernel time of the whole trace, other call sizes and warm-up included
    print(f"  sum per call: median {statistics.median(start_ns) / 1e3:.1f} us = {100 * sum(start_ns) / sum(wall_ns):.2f} % of the calls' time on their queues "
          f"(median {statistics.median(wall_ns) / 1e3:.0f} us), {100 * sum(start_ns) / all_kernel_ns:.2f} % of all kernel time")
