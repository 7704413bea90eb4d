"""Numpy FP64 restatement of the sampled-mesh signed distance (mesh_to_sdf/surface_point_cloud.py:46-54) and of the cost map
(mesh_to_sdf/depth_point_cloud.py:84-89), by chunked brute force: the construction the GPU results are pinned to.

Squared distance summed x, y, z without FMA, sqrt, cast to float32; vote dot product summed in the same order; inside when
more than half of the k nearest samples see the query behind their face.  Neighbours are ordered by (squared distance,
index): among samples at equal distance the lower index is nearer (include/gto_solver.h gto_cloud_sdf_cost).
"""
import numpy as np


def knn_rows(r, k):
    """Indices of the k + 1 first columns of every row of r in (value, index) order ((rows, k + 1); fewer columns if r has
    fewer).  argpartition finds the candidates; a row whose (k+1)-th value is tied with a later column is sorted in full."""
    n = r.shape[1]
    m = min(k + 1, n)
    if m == n:
        return np.argsort(r, axis=1, kind="stable")
    part = np.argpartition(r, m - 1, axis=1)[:, :m]
    part.sort(axis=1)  # by index, then a stable sort by value: (value, index) order
    vals = np.take_along_axis(r, part, 1)
    o = np.argsort(vals, axis=1, kind="stable")
    idx = np.take_along_axis(part, o, 1)
    thr = np.take_along_axis(vals, o, 1)[:, -1]
    tied = np.nonzero((r <= thr[:, None]).sum(axis=1) > m)[0]  # which of the tied columns argpartition kept is open
    for row in tied:
        idx[row] = np.argsort(r[row], kind="stable")[:m]
    return idx


def cloud_sdf(points, normals, query, k=11, chunk=128):
    """Returns a dict: sdf (float32, signed), inside (bool), nearest (int32), d2 (nq, min(k + 1, n)) the squared distances of
    the k + 1 nearest in order, dot (nq, k) the vote dot products of the k nearest."""
    points = np.asarray(points, dtype=np.float64)
    normals = np.asarray(normals, dtype=np.float64)
    query = np.asarray(query, dtype=np.float64).reshape(-1, 3)
    nq, m = query.shape[0], min(k + 1, points.shape[0])
    out = {"sdf": np.empty(nq, np.float32), "inside": np.empty(nq, bool), "nearest": np.empty(nq, np.int32),
           "d2": np.empty((nq, m)), "dot": np.empty((nq, k))}
    for s in range(0, nq, chunk):
        q = query[s:s + chunk]
        dx = q[:, None, 0] - points[None, :, 0]
        dy = q[:, None, 1] - points[None, :, 1]
        dz = q[:, None, 2] - points[None, :, 2]
        r = dx * dx
        r = r + dy * dy
        r = r + dz * dz
        idx = knn_rows(r, k)
        d2 = np.take_along_axis(r, idx, 1)
        near = idx[:, :k]
        ddx, ddy, ddz = (np.take_along_axis(a, near, 1) for a in (dx, dy, dz))
        nn = normals[near]
        dot = ddx * nn[..., 0]
        dot = dot + ddy * nn[..., 1]
        dot = dot + ddz * nn[..., 2]
        inside = (dot < 0).sum(axis=1) > k * 0.5
        dist = np.sqrt(d2[:, 0]).astype(np.float32)
        dist[inside] *= -1
        sl = slice(s, s + q.shape[0])
        out["sdf"][sl], out["inside"][sl], out["nearest"][sl] = dist, inside, near[:, 0]
        out["d2"][sl], out["dot"][sl] = d2, dot
    return out


def cloud_sdf_pruned(points, normals, query, k=11, extra=5):
    """cloud_sdf's dict, value for value, for many queries against a cloud of a few hundred samples: a KD-tree (scipy) names
    k + 1 + extra candidates per query, and the restatement's own arithmetic and (squared distance, index) order run on the
    candidates alone.  Why nothing is lost: a sample the tree left out is no nearer, by the tree's arithmetic, than its
    farthest candidate at distance D; the two arithmetics agree to a few 1e-16 relative, so the restatement's squared
    distance of such a sample is at least D^2 (1 - 1e-12).  A query is settled by its candidates when their (k+1)-th
    squared distance is below D^2 (1 - 1e-9): every sample left out is then strictly farther than all k + 1.  The other
    queries go through cloud_sdf.  tests/test_cloud_cases_cpu.py compares the two on a whole instance."""
    from scipy.spatial import cKDTree
    points = np.asarray(points, dtype=np.float64)
    normals = np.asarray(normals, dtype=np.float64)
    query = np.asarray(query, dtype=np.float64).reshape(-1, 3)
    m = k + 1 + extra
    if points.shape[0] <= m:
        return cloud_sdf(points, normals, query, k)
    tree = cKDTree(points)
    parts = []
    for s in range(0, max(1, query.shape[0]), 1 << 16):
        q = query[s:s + (1 << 16)]
        D, cand = tree.query(q, k=m, workers=4)
        cand = np.sort(cand, axis=1)  # by index, then a stable sort by value: (value, index) order
        dx, dy, dz = (q[:, None, a] - points[cand, a] for a in range(3))
        r = dx * dx
        r = r + dy * dy
        r = r + dz * dz
        o = np.argsort(r, axis=1, kind="stable")[:, :k + 1]
        idx = np.take_along_axis(cand, o, 1)
        d2 = np.take_along_axis(r, o, 1)
        near = idx[:, :k]
        ddx, ddy, ddz = (np.take_along_axis(a, o[:, :k], 1) for a in (dx, dy, dz))
        nn = normals[near]
        dot = ddx * nn[..., 0]
        dot = dot + ddy * nn[..., 1]
        dot = dot + ddz * nn[..., 2]
        inside = (dot < 0).sum(axis=1) > k * 0.5
        dist = np.sqrt(d2[:, 0]).astype(np.float32)
        dist[inside] *= -1
        part = {"sdf": dist, "inside": inside, "nearest": near[:, 0].astype(np.int32), "d2": d2, "dot": dot}
        open_rows = np.flatnonzero(~(d2[:, k] < D[:, -1] * D[:, -1] * (1.0 - 1e-9)))
        if len(open_rows):
            full = cloud_sdf(points, normals, q[open_rows], k)
            for name in part:
                part[name][open_rows] = full[name]
        parts.append(part)
    return {name: np.concatenate([p[name] for p in parts]) for name in parts[0]}


def cost_map(sdf, inside, epsilon=0.02, w_inside=1.0):
    """depth_point_cloud.py:84-89 in float32, the arithmetic of the device function sdf_cost_map (csrc/gto_depth.h)."""
    sdf = np.asarray(sdf, dtype=np.float32)
    eps, w = np.float32(epsilon), np.float32(w_inside)
    c = np.zeros(sdf.shape, np.float32)
    c_in = w * (-sdf + eps / np.float32(2.0))
    e = sdf - eps
    c_near = (e * e) / (np.float32(2.0) * eps)
    near = ~inside & (sdf > 0) & (sdf < eps)
    c[inside] = c_in[inside]
    c[near] = c_near[near]
    return c


def box_union_sdf(query, centers, sizes):
    """Analytic signed distance of the union of axis-aligned boxes (exact outside and inside one box; boards that touch
    make the inside value a bound, which the thin boards of a shelf never exercise beyond their thickness)."""
    q = np.asarray(query, dtype=np.float64)
    best = np.full(q.shape[0], np.inf)
    for c, s in zip(np.asarray(centers, dtype=np.float64), np.asarray(sizes, dtype=np.float64)):
        a = np.abs(q - c) - s / 2.0
        d = np.linalg.norm(np.maximum(a, 0.0), axis=1) + np.minimum(a.max(axis=1), 0.0)
        best = np.minimum(best, d)
    return best


def unpack_cloud(z, name):
    """(points, normals) of cloud `name` of tests/golden/surface_cloud.npz (normals are stored once per face)."""
    return z[f"{name}_points"], z[f"{name}_face_normals"][z[f"{name}_normal_index"]]


def unit_cube_cloud(points):
    """The cloud moved and scaled into [-0.95, 0.95]^3 (get_voxels' raster spans [-1, 1]^3; a face ON the raster's outer
    plane would put queries at distance zero from it, with a vote of exactly zero), by plain elementwise FP64."""
    lo, hi = points.min(axis=0), points.max(axis=0)
    center = (lo + hi) * 0.5
    scale = 1.9 / (hi - lo).max()
    return (points - center) * scale


def shelf_urdf_text(names, sizes, xyz):
    """An object URDF of boards (one link per board with a <box> visual, fixed to the first) from the recorded sizes and
    visual origins of the fixture."""
    fmt = lambda v: " ".join(repr(float(x)) for x in v)
    links = "".join(f'<link name="{n}"><visual><origin rpy="0 0 0" xyz="{fmt(o)}"/><geometry><box size="{fmt(s)}"/></geometry>'
                    f'</visual></link>' for n, s, o in zip(names, sizes, xyz))
    joints = "".join(f'<joint name="fixed_joint{i}" type="fixed"><parent link="{names[0]}"/><child link="{n}"/>'
                     f'<origin rpy="0 0 0" xyz="0 0 0"/></joint>' for i, n in enumerate(names[1:], 1))
    return f'<?xml version="1.0"?><robot name="shelf">{links}{joints}</robot>'
