"""Edge clouds for the sampled-mesh kernels (grasptrajopt_amd/csrc/gto_cloud.h, the cloud half of gto_observe.h): plain numpy,
no GPU (the plan part at the end takes robot descriptions through depth_cases.plan_robot, numpy too).

The kernels keep four kinds of books: a list of 1, 12 or 16 best samples per lane (GTO_CLOUD_DISPATCH, CloudBest::kth), runs
of 32 Morton-sorted samples under a complete binary tree of a power of two of leaf slots (k_query_keys, k_cloud_gather,
k_cloud_leaves, k_bvh_up), the skip test `box distance <= kth` of the packet walk (k_cloud_knn), and chunks of at most 2^24
queries per launch chain of a check (chunk_items in gto_api.hip).  cases() puts a cloud on every place where one of them
changes its path; posed_instance() and plan_cloud() build what the two collision checks are asked on them.  The expected
values are cloud_sdf_ref.cloud_sdf / cost_map (brute force in FP64, (squared distance, index) order) and, for the plans,
the FP64 oracle's world points put through cloud_sdf.  sample_leaves() restates the key formula of the sample sort where a
test has to know which leaf a sample lands in, and single_lane_walk() the walk of a query asked alone, with `<=` or `<` in
its skip tests: lattice_witnesses() are the queries that tell the two apart.  tests/test_cloud_cases_cpu.py holds the cases to
what this text claims.

  name               n       leaves / slots   what it is for
  n_equals_k_<k>     k       1 / 1            k = 1, 2, 11, 12, 13, 16: a list exactly as long as the cloud; the two edges of
                                              the dispatch (12: the 12-list full, 13: the smallest k of the 16-list)
  leaf_shapes_32     32      1 / 1            one full leaf, no inner node: k_bvh_up is not launched
  leaf_shapes_257    257     9 / 16           an entirely empty subtree (slots 12-15 and their parents)
  leaf_shapes_2049   2049    65 / 128         one leaf past a power of two: half the tree empty
  all_same           40      2 / 2            one point 40 times: every distance ties, the k lowest indices win; normals
                                              alternate +z, -z by index so that the vote shows which indices won; every box has
                                              zero extent, every key is 0; more copies than GTO_CLOUD_MAX_K
  duplicates         1000    32 / 32          50 points 20 times each, sample c * 50 + j = copy c of point j: equal keys, so the
                                              stable sort lays the 20 copies side by side in index order, across leaf borders
  collinear          300     10 / 16          on a line along x: zero extent in y and z (k_query_keys: ext > 0 ? ... : 0)
  coplanar           1024    32 / 32          a 32 x 32 lattice in z = 0.25, spacing 1/64: zero extent in z; four equidistant
                                              samples at a cell centre
  lattice3d          512     16 / 16          8 x 8 x 8, spacing 1/8, indices shuffled: ties between samples of different
                                              leaves at exactly the k-th distance (the `<=` of the skip test)
  far_apart          200     7 / 8            two clusters 1e6 m apart, spacing 1e-3 m: two key cells along x, a leaf that spans both
  scattered          20000   625 / 1024       random, with 1000 queries in random order: the walk without `order`

Coordinates that have to tie are binary fractions, so the squared distances tie exactly in FP64.  Query counts are no
multiples of 64 (one is 1)."""
from types import SimpleNamespace

import numpy as np

import cloud_sdf_ref as ref
import depth_cases as dc

LEAF = 32  # GTO_CLOUD_LEAF
MAX_K = 16  # GTO_CLOUD_MAX_K
KS = (1, 2, 11, 12, 13, 16)  # CloudBest<1>; <12> at its first, its usual and its last k; <16> at its first and last k
CHUNK_QUERIES = 1 << 24  # kCheckChunkQueries (gto_api.hip)
TIE_CASES = ["all_same", "duplicates", "collinear", "coplanar", "lattice3d"]
ZERO_EXTENT = {"all_same": (0, 1, 2), "collinear": (1, 2), "coplanar": (2,)}
LATTICE_SEED = 0  # the permutation of lattice3d (tests/test_cloud_cases_cpu.py: a cross-leaf tie at the k-th distance for every k)


# ------------------------------------------------------------------------------------------ the sample sort, restated
def _part1by2(v):
    v = v.astype(np.uint32) & np.uint32(0x3ff)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000ff)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300f00f)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030c30c3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def sample_keys(points):
    """The 30-bit Morton keys make_sample_cloud gives the samples (gto_api.hip, k_query_keys in gto_depth.h): k_query_keys
    spreads a box grown by its own extent over the key range, and is handed the middle third of the bounding box."""
    p = np.asarray(points, dtype=np.float64)
    lo, hi = p.min(0), p.max(0)
    key = np.zeros(len(p), np.uint32)
    for a in range(3):
        third = (hi[a] - lo[a]) / 3.0
        klo, khi = lo[a] + third, hi[a] - third
        ext = khi - klo
        u = (p[:, a] - (klo - ext)) / (3.0 * ext) if (ext > 0.0 and ext < np.inf) else np.zeros(len(p))
        u = np.minimum(np.maximum(u, 0.0), 1.0)
        key |= _part1by2((u * 1023.0).astype(np.uint32)) << np.uint32(a)
    return key


def sample_leaves(points):
    """Leaf of every sample: a stable sort by key (the radix sort of (key, index) is one), 32 consecutive samples per leaf."""
    order = np.argsort(sample_keys(points), kind="stable")
    leaf = np.empty(len(order), np.int64)
    leaf[order] = np.arange(len(order)) // LEAF
    return leaf


def leaf_slots(n):
    """(leaves in use, leaf slots of the tree): cloud_leaf_slots of gto_cloud.h."""
    leaves = -(-n // LEAF)
    p = 1
    while p < leaves:
        p <<= 1
    return leaves, p


def single_lane_walk(points, q, k, strict=False):
    """k_cloud_knn's walk for a launch of ONE query (a packet with one live lane, so no other lane's need opens a box for it),
    restated: indices of the k best in order.  Heap-indexed boxes over the sorted samples (k_cloud_leaves, k_bvh_up), the
    nearer child first (c1 when d1 <= d2), a box taken when its distance is <= kth both when it is pushed and when it is
    popped, all 32 samples of a leaf offered to a list of 1, 12 or 16 entries in (squared distance, index) order.
    strict=True is the walk with `<` in both skip tests: what the `<=` is compared with."""
    p = np.asarray(points, dtype=np.float64)
    order = np.argsort(sample_keys(p), kind="stable")
    leaves, slots = leaf_slots(len(p))
    lo, hi = np.full((2 * slots, 3), np.inf), np.full((2 * slots, 3), -np.inf)
    for l in range(leaves):
        run = p[order[l * LEAF:(l + 1) * LEAF]]
        lo[slots - 1 + l], hi[slots - 1 + l] = run.min(0), run.max(0)
    for node in range(slots - 2, -1, -1):
        lo[node], hi[node] = np.minimum(lo[2 * node + 1], lo[2 * node + 2]), np.maximum(hi[2 * node + 1], hi[2 * node + 2])

    def box_d2(node):
        e = np.maximum(np.maximum(lo[node] - q, q - hi[node]), 0.0)
        return float((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])

    cap = 1 if k <= 1 else (12 if k <= 12 else 16)  # GTO_CLOUD_DISPATCH
    best, kth, stack = [], np.inf, [0]
    takes = (lambda d: d < kth) if strict else (lambda d: d <= kth)
    while stack:
        node = stack.pop()
        if not takes(box_d2(node)):
            continue
        if node >= slots - 1:
            ids = order[(node - slots + 1) * LEAF:(node - slots + 2) * LEAF]
            d = q - p[ids]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            best = sorted(best + list(zip(d2.tolist(), ids.tolist())))[:cap]
            kth = best[k - 1][0] if len(best) >= k else np.inf
        else:
            c1, c2 = 2 * node + 1, 2 * node + 2
            d1, d2 = box_d2(c1), box_d2(c2)
            first, second = (c1, c2) if d1 <= d2 else (c2, c1)
            for c in (second, first):
                if takes(box_d2(c)):
                    stack.append(c)
    return [i for _, i in best[:k]]


_WITNESSES = None


def lattice_witnesses():
    """{k: rows of lattice3d's queries}: the queries on which the walk with `<` in the skip tests, asked alone, returns other
    neighbours than the restatement, because a box AT the k-th distance holds a tying sample of lower index than one the
    list already has.  (The walk with `<=` returns the restatement's on every query: tests/test_cloud_cases_cpu.py.)"""
    global _WITNESSES
    if _WITNESSES is None:
        c = cases()["lattice3d"]
        idx = np.argsort(squared_distances(c.points, c.query), axis=1, kind="stable")
        _WITNESSES = {k: [row for row in range(len(c.query)) if single_lane_walk(c.points, c.query[row], k, strict=True) != idx[row, :k].tolist()]
                      for k in KS}
    return _WITNESSES


STATED_LEAVES = {"n_equals_k_1": (1, 1), "n_equals_k_2": (1, 1), "n_equals_k_11": (1, 1), "n_equals_k_12": (1, 1), "n_equals_k_13": (1, 1),
                 "n_equals_k_16": (1, 1), "leaf_shapes_32": (1, 1), "leaf_shapes_257": (9, 16), "leaf_shapes_2049": (65, 128),
                 "all_same": (2, 2), "duplicates": (32, 32), "collinear": (10, 16), "coplanar": (32, 32), "lattice3d": (16, 16),
                 "far_apart": (7, 8), "scattered": (625, 1024)}


# ------------------------------------------------------------------------------------------ the clouds
def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _n_equals_k(k, rng):
    nq = {1: 1, 2: 63, 11: 65, 12: 129, 13: 257, 16: 191}[k]
    pts = rng.uniform(-0.3, 0.3, (k, 3))
    q = np.concatenate([pts[:1], rng.uniform(-0.5, 0.5, (nq - 1, 3))])
    return pts, rng.normal(size=(k, 3)), q, (k,)


def _leaf_shapes(n, rng):
    pts = rng.uniform(-0.3, 0.3, (n, 3))
    q = np.concatenate([rng.uniform(-0.4, 0.4, (300, 3)), pts[:5], 50.0 + rng.normal(size=(10, 3))])
    return pts, rng.normal(size=(n, 3)), q, KS


def _all_same(rng):
    p = np.array([0.375, -0.25, 0.5])
    pts = np.tile(p, (40, 1))
    nrm = np.tile([0.0, 0.0, 1.0], (40, 1)) * np.where(np.arange(40) % 2 == 0, 1.0, -1.0)[:, None]
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    q = np.concatenate([p[None], p + 0.125 * axes, p + 4.0 * axes, p + rng.uniform(-0.2, 0.2, (54, 3))])
    return pts, nrm, q, KS


def _duplicates(rng):
    base = np.round(rng.uniform(-0.3, 0.3, (50, 3)) * 1024) / 1024
    bn = rng.normal(size=(50, 3))
    pts = np.tile(base, (20, 1))  # sample c * 50 + j is copy c of point j
    c = np.repeat(np.arange(20), 50)
    nrm = np.tile(bn, (20, 1)) * np.where(c % 3 == 0, 1.0, -1.0)[:, None] + 0.01 * c[:, None]
    q = np.concatenate([base, (base[:25] + base[25:]) / 2, rng.uniform(-0.4, 0.4, (120, 3))])
    return pts, nrm, q, KS


def _collinear(rng):
    x = rng.permutation(300) / 256.0
    pts = np.stack([x, np.full(300, 0.5), np.full(300, -0.25)], axis=1)
    on = pts[:40]
    mid = np.stack([(np.arange(40) * 7 + 0.5) / 256.0, np.full(40, 0.5), np.full(40, -0.25)], axis=1)  # between two samples
    off = mid + np.array([0.0, 0.0625, -0.03125])  # the same, off the line: two equidistant samples still
    q = np.concatenate([on, mid, off, rng.uniform(-0.2, 1.4, (70, 3)) * [1.0, 0.3, 0.3] + [0.0, 0.35, -0.4]])
    return pts, rng.normal(size=(300, 3)), q, KS


def _coplanar(rng):
    g = np.arange(32) / 64.0
    pts = np.stack(list(np.meshgrid(g, g, indexing="ij")) + [np.full((32, 32), 0.25)], axis=-1).reshape(-1, 3)
    pts = pts[rng.permutation(len(pts))]
    ij = rng.integers(2, 29, (120, 2))
    node = np.concatenate([ij[:40] / 64.0, np.full((40, 1), 0.25)], axis=1)
    centre = np.concatenate([(ij[40:80] + 0.5) / 64.0, np.full((40, 1), 0.25)], axis=1)  # in the plane: every vote is 0
    above = np.concatenate([(ij[80:] + 0.5) / 64.0, np.where(np.arange(40) % 2 == 0, 0.25 + 0.0625, 0.25 - 0.03125)[:, None]], axis=1)
    q = np.concatenate([node, centre, above, rng.uniform(-0.1, 0.6, (77, 3))])
    return pts, rng.normal(size=(len(pts), 3)), q, KS


def _lattice3d(rng):
    g = np.arange(8) / 8.0
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = pts[np.random.default_rng(LATTICE_SEED).permutation(512)]  # index order is not spatial order
    i3 = rng.integers(2, 6, (150, 3))  # interior: the shells of equidistant samples around them are complete
    node = i3[:50] / 8.0
    face = (i3[50:100] + [0.5, 0.5, 0.0]) / 8.0
    face[::2] = face[::2, [2, 0, 1]]
    cell = (i3[100:] + 0.5) / 8.0
    q = np.concatenate([node, face, cell, rng.uniform(-0.1, 1.0, (49, 3))])
    return pts, rng.normal(size=(512, 3)), q, KS


def _far_apart(rng):
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(4), indexing="ij"), axis=-1).reshape(-1, 3) * 1.0e-3
    other = np.array([1.0e6, 0.0, 0.0])
    pts = np.concatenate([g, g + other])[rng.permutation(200)]
    near = lambda c, m: c + rng.uniform(-0.01, 0.01, (m, 3))
    q = np.concatenate([near(np.zeros(3), 40), near(other, 40), other / 2 + rng.uniform(-1.0, 1.0, (10, 3)), g[:5], g[5:10] + other,
                        [other / 2 + [0.002, 0.002, 0.0015]]])  # (the last one: half-way between the clusters' centres)
    return pts, rng.normal(size=(200, 3)), q, KS


def _scattered(rng):
    pts = rng.random((20000, 3))
    nrm = _unit(rng.normal(size=(20000, 3)))
    q = np.concatenate([rng.uniform(-0.2, 1.2, (700, 3)), pts[:200] + rng.normal(scale=1e-3, size=(200, 3)), pts[200:300]])
    return pts, nrm, q[rng.permutation(1000)], (1, 11, 13)  # consecutive queries are far apart


_CASES = None


def cases():
    """{name: case}; a case has name, points (n, 3), normals (n, 3), query (nq, 3), ks (the k to run), epsilon, w_inside."""
    global _CASES
    if _CASES is None:
        makers = [(f"n_equals_k_{k}", lambda r, k=k: _n_equals_k(k, r)) for k in KS]
        makers += [(f"leaf_shapes_{n}", lambda r, n=n: _leaf_shapes(n, r)) for n in (32, 257, 2049)]
        makers += [("all_same", _all_same), ("duplicates", _duplicates), ("collinear", _collinear), ("coplanar", _coplanar),
                   ("lattice3d", _lattice3d), ("far_apart", _far_apart), ("scattered", _scattered)]
        _CASES = {}
        for i, (name, make) in enumerate(makers):
            pts, nrm, q, ks = make(np.random.default_rng(5200 + i))
            pts, nrm, q = (np.ascontiguousarray(a, dtype=np.float64) for a in (pts, nrm, q))
            for a in (pts, nrm, q):
                a.setflags(write=False)
            _CASES[name] = SimpleNamespace(name=name, points=pts, normals=nrm, query=q, ks=tuple(ks),
                                           epsilon=(0.03, 0.05, 0.02)[i % 3], w_inside=(2.0, 1.0, 1.5)[i % 3])
    return _CASES


_EXPECTED = {}


def _frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


def expected(name, k):
    """cloud_sdf of a case at its own queries with `cost` added: computed once and left unchanged."""
    if (name, k) not in _EXPECTED:
        c = cases()[name]
        with np.errstate(all="ignore"):
            out = ref.cloud_sdf(c.points, c.normals, c.query, k=k)
        out["cost"] = ref.cost_map(out["sdf"], out["inside"], c.epsilon, c.w_inside)
        _EXPECTED[(name, k)] = _frozen(out)
    return _EXPECTED[(name, k)]


def squared_distances(points, query):
    """(nq, n): the restatement's squared distances (summed x, y, z)."""
    d = [query[:, None, a] - points[None, :, a] for a in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


# ------------------------------------------------------------------------------------------ non-finite queries
def nonfinite_queries(case):
    """(query with 12 bad rows spread among the case's first 130 queries, bad_at their rows, finite_at the others' rows, kinds):
    kinds[i] is "nan" (a NaN coordinate, with or without an infinite one beside it) or "inf" (an infinite one and no NaN)."""
    inf, nan = np.inf, np.nan
    bad = np.array([[nan, 0.1, 0.2], [0.1, nan, 0.2], [0.1, 0.2, nan], [nan, nan, nan], [inf, nan, 0.0], [inf, 0.1, 0.2],
                    [0.1, -inf, 0.2], [0.1, 0.2, inf], [inf, inf, inf], [-inf, inf, 0.0], [-inf, -inf, -inf], [inf, 0.0, -0.0]])
    kinds = ["nan"] * 5 + ["inf"] * 7
    good = case.query[:130]
    bad_at = np.array([0, 1, 40, 63, 64, 65, 100, 127, 128, 129, 140, 141])
    q = np.empty((len(good) + len(bad), 3))
    finite_at = np.setdiff1d(np.arange(len(q)), bad_at)
    q[bad_at], q[finite_at] = bad, good
    return q, bad_at, finite_at, kinds


def lowest_indices_vote(case, q, k):
    """inside of a query at infinity: the vote of samples 0 .. k - 1, the restatement's dot product."""
    with np.errstate(all="ignore"):
        d = q[None, :] - case.points[:k]
        dot = (d[:, 0] * case.normals[:k, 0] + d[:, 1] * case.normals[:k, 1]) + d[:, 2] * case.normals[:k, 2]
    return bool((dot < 0).sum() > k * 0.5)


# ------------------------------------------------------------------------------------------ scene grids
MAX_VOXELS = 10000  # (the field stays far under 40 000 voxels: the restatement visits every voxel-sample pair)
SCENE_CLOUDS = [("coplanar", 11), ("leaf_shapes_257", 12), ("duplicates", 13)]  # name, k


def planner_grid(points, res, margin):
    """gto/gto_models.py:155-171: shape, origin and voxel centres (C order) of the grid around the cloud."""
    lo, hi = points.min(0), points.max(0)
    axes = [np.arange(lo[a] - margin, hi[a] + margin, res) for a in range(3)]
    wp = np.array(np.meshgrid(*axes, indexing="ij"))
    return wp.shape[1:], np.array([lo[a] - margin for a in range(3)]), wp.reshape((3, -1)).T


def scene_cases():
    """name, case, k, n_obstacle, grid_res, margin, epsilon, w_inside: every cloud of SCENE_CLOUDS with n_obstacle = k,
    n_all - 1 and n_all, a margin of 0.1 m and the resolution (a multiple of 5 mm from 2 cm) that keeps the grid under
    MAX_VOXELS; epsilon is 0.05 m, more than a voxel.  coplanar's z axis is the margin alone."""
    out = []
    for name, k in SCENE_CLOUDS:
        c = cases()[name]
        ext = c.points.max(0) - c.points.min(0)
        margin, res = 0.1, 0.02
        while np.prod(np.ceil((ext + 2 * margin) / res) + 1) > MAX_VOXELS:
            res += 0.005
        for n_obs in (k, len(c.points) - 1, len(c.points)):
            out.append(SimpleNamespace(name=f"{name}-{n_obs}", case=c, k=k, n_obstacle=n_obs, grid_res=float(res), margin=margin,
                                       epsilon=0.05, w_inside=1.5))
    return out


_FIELDS = {}


def scene_field(sc, n):
    """cost_map(cloud_sdf) of the first n samples of the scene's cloud at its voxel centres, computed once."""
    key = (sc.case.name, n)
    if key not in _FIELDS:
        c = sc.case
        q = planner_grid(c.points, sc.grid_res, sc.margin)[2]
        out = ref.cloud_sdf(c.points[:n], c.normals[:n], q, k=sc.k, chunk=512)
        cost = ref.cost_map(out["sdf"], out["inside"], sc.epsilon, sc.w_inside)
        cost.setflags(write=False)
        _FIELDS[key] = (cost, out["inside"])
    return _FIELDS[key]


# ------------------------------------------------------------------------------------------ gripper points and poses
POSED_CASES = ["leaf_shapes_257", "scattered"]
POSED_KS = (1, 11)
CHUNK_POSED = SimpleNamespace(P=4096, n=4097, n_samples=33, k=11)  # 4096 * 4096 = 2^24: pose 4096 goes into a second chain


def posed_instance(case, n_points, n_poses=6):
    """Gripper points (n_points, 3) around the origin and poses (n_poses, 4, 4), built as depth_cases.posed_instance builds them:
    a small turn about a random axis and a shift onto one of the case's queries (one within the cloud's bounding box, so
    that the samples around decide).  Pose 2 holds a NaN."""
    rng = np.random.default_rng(900 + n_points)
    pts = rng.uniform(-0.08, 0.08, (n_points, 3))
    lo, hi = case.points.min(0), case.points.max(0)
    within = np.flatnonzero(((case.query >= lo) & (case.query <= hi)).all(axis=1))
    RT = np.tile(np.eye(4), (n_poses, 1, 1))
    for i in range(n_poses):
        w = rng.standard_normal(3)
        w /= np.linalg.norm(w)
        a = rng.uniform(-0.6, 0.6)
        Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        RT[i, :3, :3] = np.eye(3) + np.sin(a) * Wx + (1 - np.cos(a)) * Wx @ Wx
        RT[i, :3, 3] = case.query[within[rng.integers(len(within))]]
    RT[2, 1, 3] = np.nan
    return pts, RT


_POSED = {}


def posed_expected(points, normals, pts, RT, k):
    """int32 (n_poses,): the restated count per pose, -1 for a pose with a non-finite entry."""
    bad = ~np.isfinite(RT).all(axis=(1, 2))
    world = dc.placed(pts, np.where(bad[:, None, None], np.eye(4), RT))
    inside = ref.cloud_sdf(points, normals, world.reshape(-1, 3), k=k)["inside"].reshape(len(RT), len(pts))
    return np.where(bad, -1, inside.sum(axis=1)).astype(np.int32)


def posed_counts(name, n_points, k):
    """(pts, RT, expected counts) of posed_instance on case `name`, computed once."""
    if (name, n_points, k) not in _POSED:
        c = cases()[name]
        pts, RT = posed_instance(c, n_points)
        want = posed_expected(c.points, c.normals, pts, RT, k)
        want.setflags(write=False)
        _POSED[(name, n_points, k)] = (pts, RT, want)
    return _POSED[(name, n_points, k)]


def chunk_posed_instance():
    """The second-chunk instance of check_posed: a cloud of 33 samples (two leaves), 4096 gripper points, 4097 poses that
    cycle through six (pose 2 of them holds a NaN).  Returns points, normals, pts, poses (4097, 4, 4), expected (4097,)."""
    s = CHUNK_POSED
    rng = np.random.default_rng(33)
    points, normals = rng.uniform(-0.3, 0.3, (s.n_samples, 3)), rng.normal(size=(s.n_samples, 3))
    c = SimpleNamespace(points=points, query=rng.uniform(-0.25, 0.25, (20, 3)))
    pts, six = posed_instance(c, s.P)
    want6 = posed_expected(points, normals, pts, six, s.k)
    pick = np.arange(s.n) % 6
    return points, normals, pts, six[pick], want6[pick]


# ------------------------------------------------------------------------------------------ plans against a box of samples
PLAN_K = 11
SPACING, JITTER = 0.02, 0.003
TOL = 1e-9  # a decision closer than this could fall the other way on the device's kinematics (depth_cases.undecided)
PLAN_SEED = {("panda", 96): 1, ("bushy8", 22): 1, ("bushy8", 50): 1, ("bushy8", 96): 2, ("chain16", 96): 4}  # where the seeds below left an undecided point


def box_samples(lo, hi, rng):
    """The six faces of the box [lo, hi] (its sides multiples of SPACING) sampled on a jittered lattice: one sample per
    SPACING x SPACING cell, at the cell's centre moved by at most JITTER within the face.  Normals point outward."""
    pts, nrm = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        nb, nc = int(round((hi[b] - lo[b]) / SPACING)), int(round((hi[c] - lo[c]) / SPACING))
        ub, uc = np.meshgrid(lo[b] + (np.arange(nb) + 0.5) * SPACING, lo[c] + (np.arange(nc) + 0.5) * SPACING, indexing="ij")
        for side, sign in ((lo[a], -1.0), (hi[a], 1.0)):
            p = np.empty((nb * nc, 3))
            p[:, a] = side
            p[:, b] = ub.reshape(-1) + rng.uniform(-JITTER, JITTER, nb * nc)
            p[:, c] = uc.reshape(-1) + rng.uniform(-JITTER, JITTER, nb * nc)
            n = np.zeros((nb * nc, 3))
            n[:, a] = sign
            pts.append(p)
            nrm.append(n)
    return np.concatenate(pts), np.concatenate(nrm)


def plan_cloud(name, desc, T, world_points, seed=None, key=None):
    """The plans of depth_cases.plan_instance (B = 3 straight joint-space plans, a shared base, per-plan bases, a NaN to plant)
    and an obstacle for them: a closed axis-aligned box around where the second half of plan 0 puts the robot's far links
    (the tenth of its surface points farthest from the base at the last waypoint), under the shared base and under plan 0's
    own.  The box spans the middle half of these positions per axis, is at least 8 cm and at most 16 cm wide and is snapped
    outward to multiples of SPACING; its faces are sampled by box_samples.  Numpy alone.  Returns the instance with points,
    normals, lo, hi added."""
    if seed is None:
        seed = PLAN_SEED.get((name, T), 0)
    inst = dc.plan_instance(name, desc, T, world_points, key=key)
    rng = np.random.default_rng(8000 + 100 * (dc.PLAN_ROBOTS.index(name) if key is None else key) + T + 1000 * seed)
    ts = np.arange((T - 1) // 2 + 1, T)
    q = inst.plans[0][:, ts].T
    xa = world_points(q, np.tile(inst.base, (len(ts), 1)))
    xb = world_points(q, np.tile(inst.bases[0], (len(ts), 1)))
    P = xa.shape[1]
    far = np.argsort(np.linalg.norm(xa[-1] - inst.base, axis=1))[-max(8, P // 10):]
    S = np.concatenate([xa[:, far], xb[:, far]]).reshape(-1, 3)
    q1, q3 = np.quantile(S, 0.25, axis=0), np.quantile(S, 0.75, axis=0)
    mid, half = (q1 + q3) / 2, np.clip((q3 - q1) / 2, 0.04, 0.08)
    lo, hi = np.floor((mid - half) / SPACING) * SPACING, np.ceil((mid + half) / SPACING) * SPACING
    inst.points, inst.normals = box_samples(lo, hi, rng)
    inst.lo, inst.hi = lo, hi
    return inst


def undecided(out, k, tol=TOL):
    """Queries of a cloud_sdf result whose vote a change of `tol` in their position could turn: the k-th and (k+1)-th nearest
    samples within tol of each other in distance, or enough dot products within tol of zero to turn the majority."""
    d2, dot = out["d2"], out["dot"]
    close = np.sqrt(d2[:, k]) - np.sqrt(d2[:, k - 1]) <= tol if d2.shape[1] > k else np.zeros(len(d2), bool)
    votes = (dot < 0).sum(axis=1)
    near = np.abs(dot) <= tol
    could_leave = votes - (near & (dot < 0)).sum(axis=1)   # votes left when every near one falls the other way
    could_join = votes + (near & ~(dot < 0)).sum(axis=1)
    inside = votes > k * 0.5
    return close | (inside & ~(could_leave > k * 0.5)) | (~inside & (could_join > k * 0.5))


def plan_expected(inst, desc, world_points, bases):
    """(counts (B, T) int32 with -1 at the NaN waypoint, number of undecided points) for the plans of `inst` with the NaN
    planted, at bases (3,) or (B, 3): the oracle's points through cloud_sdf, k = PLAN_K."""
    B, T = dc.PLAN_B, inst.T
    b3 = np.broadcast_to(np.asarray(bases, dtype=np.float64).reshape(-1, 3), (B, 3))
    q = inst.plans.transpose(0, 2, 1).reshape(B * T, desc.ndof)
    xyz = world_points(q, np.repeat(b3, T, axis=0)).reshape(-1, 3)
    out = ref.cloud_sdf_pruned(inst.points, inst.normals, xyz, k=PLAN_K)
    counts = out["inside"].reshape(B, T, -1).sum(axis=2).astype(np.int32)
    und = undecided(out, PLAN_K).reshape(B, T, -1)
    p, _, t = inst.nan_at
    counts[p, t] = -1
    und[p, t] = False
    return counts, int(und.sum())


_PLANS = {}


def plan_case(name, T, desc, world_points):
    """plan_cloud and its expected counts under the shared base and under the per-plan bases, computed once per (robot, T):
    (inst, {"shared": (counts, n_undecided), "per_plan": (counts, n_undecided)})."""
    if (name, T) not in _PLANS:
        inst = plan_cloud(name, desc, T, world_points)
        want = {"shared": plan_expected(inst, desc, world_points, inst.base), "per_plan": plan_expected(inst, desc, world_points, inst.bases)}
        for c, _ in want.values():
            c.setflags(write=False)
        _PLANS[(name, T)] = (inst, want)
    return _PLANS[(name, T)]


CHUNK_PLANS = SimpleNamespace(robot="chain16", T=96)


def chunk_plans_B(P, T=96):
    """One plan more than a launch chain of gto_check_plans takes at T * P queries per plan."""
    return CHUNK_QUERIES // (T * P) + 1
