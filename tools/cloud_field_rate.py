#!/usr/bin/env python3
"""cloud_field_rate.py — time of one gto_scene_from_clouds call on the shelf scene (the six boards of
tests/golden/surface_cloud.npz with a box on the middle board: two fields) at about 128^3 voxels x {1e5, 3e5, 1e6}
samples, k = 11 and k = 1, tree search and exhaustive search (GTO_CLOUD_BRUTE).  Median of five timed calls after one
warm-up call; a call ends with the device synchronised.  One further call per row under GTO_CLOUD_STATS makes the
library print its own split (upload | sort + build | queries, keys, sort | search | records) on stderr.
    python tools/cloud_field_rate.py [--samples N ...] [--commit TEXT] 2> split.txt"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402  (lib_sha16)
import cloud_sdf_ref as ref  # noqa: E402
from grasptrajopt_amd import _capi, load_builtin  # noqa: E402
from grasptrajopt_amd import surface_point_cloud as spc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, nargs="*", default=[100000, 300000, 1000000])
ap.add_argument("--voxels", type=float, default=128.0 ** 3)
ap.add_argument("--commit", default="unknown")
a = ap.parse_args()

z = np.load(os.path.join(ROOT, "tests", "golden", "surface_cloud.npz"))
parts = [(m, T) for _, m, T in spc.urdf_visual_meshes(ref.shelf_urdf_text(z["shelf_names"], z["shelf_box_size"], z["shelf_box_xyz"]))]
box_pose = np.eye(4)
box_pose[:3, 3] = [0.1, 0.0, 0.3905 + 0.011 + 0.05]
parts.append((spc.box_mesh([0.05, 0.05, 0.1]), box_pose))
area = np.array([spc.mesh_area(*m) for m, _ in parts])
margin = 0.4
ext = (z["shelf_vertices"].max(0) - z["shelf_vertices"].min(0)) + 2 * margin
res = float((ext.prod() / a.voxels) ** (1.0 / 3.0))
h = _capi.SolverHandle(load_builtin("panda"), "panda_hand", "panda_hand", device=0)
print(f"# tools/cloud_field_rate.py on one MI355X; commit {a.commit}, lib_sha16 {bench.lib_sha16()}")
print(f"# shelf (6 boards) + box, grid_res {res:.5f} m, margin {margin} m; ms per gto_scene_from_clouds call (two fields), median of 5 [min .. max]")
for n in a.samples:
    counts = np.ceil(n * area / area.sum()).astype(int)
    pts, nrm = spc.place_meshes(parts, counts=counts, seed=0)
    n_obs = int(counts[:-1].sum())
    for k in (11, 1):
        fields = {}
        for mode in ("tree", "exhaustive"):
            os.environ.pop("GTO_CLOUD_STATS", None)
            os.environ["GTO_CLOUD_BRUTE"] = "1" if mode == "exhaustive" else "0"
            shape, _, _ = h.scene_from_clouds(0, pts, nrm, n_obs, k, res, margin)
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                h.scene_from_clouds(0, pts, nrm, n_obs, k, res, margin)
                ts.append(1e3 * (time.perf_counter() - t0))
            os.environ["GTO_CLOUD_STATS"] = "1"
            h.scene_from_clouds(0, pts, nrm, n_obs, k, res, margin)
            fields[mode] = h.scene_fields(0)
            print(f"samples {len(pts):8d}  voxels {int(np.prod(shape)):8d} {tuple(shape)}  k {k:2d}  {mode:10s} "
                  f"{statistics.median(ts):10.2f} ms  [{min(ts):.2f} .. {max(ts):.2f}]", flush=True)
        same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(fields["tree"], fields["exhaustive"]))
        print(f"    tree == exhaustive bit for bit: {same}; voxels with a cost: {int((fields['tree'][0] > 0).sum())}", flush=True)
h.close()
