"""Edge image shapes for the depth-image kernels (grasptrajopt_amd/csrc/gto_depth.h, gto_observe.h): plain numpy, no GPU
(the plan part at the end also takes robot descriptions from tests/helpers.py and grasptrajopt_amd.robot_desc, numpy too).

The kernels keep three kinds of books: tiles of 8 x 4 pixels in Morton order under a complete binary tree of P x P leaf
slots (k_bvh_leaves, k_bvh_up; P = tile_levels(H, W), a power of two), queries 64 to a wave in the order of 30-bit keys
(k_query_keys, k_depth_sdf_bvh) and workgroups of four waves (k_depth_sdf, k_check_posed, k_check_plans).  cases() puts
an image on every size at which one of them changes its path, scene_cases() sizes a workspace grid for the cost-only
search of gto_scene_from_depth around the small ones, plan_instance() builds an image for a robot's plans to reach through.
The expected values are the FP64 oracle's (oracle/gto_oracle.c); backproject() and project() restate its two formulas
term for term where a generator or a test needs an intermediate the oracle does not hand out (the cloud's points to put a
query on, pixel coordinates to tell how far a point is from a decision).  tests/test_depth_cases_cpu.py holds the
restatements to the oracle and the cases to what this text claims.

  name            H x W     P     what it crosses
  one_pixel       1 x 1     1     the root is the leaf, k_bvh_up is not launched; one cloud point
  one_tile        4 x 8     1     the same with a full tile; nq = 1
  under_tile      3 x 5     1     the same with a ragged tile
  tile_plus_one   5 x 9     2     three of the four leaves hold one row or one column of pixels
  row_strip       1 x 200   32    25 of 1024 leaf slots filled: one row of tiles, each holding one row of pixels
  col_strip       130 x 1   64    33 of 4096 leaf slots filled: one column of tiles, each holding one column of pixels
  pow2_full       32 x 64   8     8 x 8 tiles: every leaf slot full
  pow2_over       33 x 65   16    9 x 9 tiles: one over the power of two; a few thousand queries
  widest_tree     1 x 8192  1024  the last size k_bvh_up builds
  past_the_tree   1 x 8200  2048  beyond it: the exhaustive kernel (gto_depth_sdf_cost, observation), a refusal (scene)
  single_valid    33 x 65   16    one valid pixel (the others 0 or beyond the threshold): a root box of zero extent, every key 0
  none_valid      12 x 20   4     no valid pixel: an empty root box, every distance infinite
  holes           33 x 65   16    dead tiles, masked tiles, a stripe beyond the threshold, one live pixel among dead tiles
  flat_wall       20 x 40   8     identity camera rotation, constant depth: the cloud's z extent is exactly 0

Queries of a case, shuffled: half of them in two boxes around the cloud (one reaching behind the camera and out of the
viewport), a third through pixel coordinates of which half lie in (-1, 0) (truncation toward zero puts them into column
or row 0), an eighth exactly on cloud points (distance 0: the sign alone decides between +0.0f and -0.0f), four at
1e6 m and, for flat_wall, eight with camera-frame z exactly 0 (a division by zero: the pixel index is LONG_MIN).  The
counts between them: 1, 63, 64, 65, 255, 256, 257 (a wave, a workgroup, one under and one over) and 1000 to 3000.
"""
from types import SimpleNamespace

import numpy as np

TILE_W, TILE_H, MAX_P = 8, 4, 1024  # GTO_BVH_TILE_W, GTO_BVH_TILE_H, GTO_BVH_MAX_P


def tile_levels(H, W):
    """gto_depth.h tile_levels: leaf slots per side of the hierarchy of an H x W image."""
    tx, ty = (W + TILE_W - 1) // TILE_W, (H + TILE_H - 1) // TILE_H
    P = 1
    while P < tx or P < ty:
        P <<= 1
    return P


# ------------------------------------------------------------------------------------------ the oracle's two formulas
def backproject(depth, K, cam, mask, threshold):
    """orc_depth_backproject term for term: (points (H*W, 3) in pixel order, valid (H*W,) bool)."""
    H, W = depth.shape
    Kinv = np.linalg.inv(K)
    y, x = (a.reshape(-1).astype(np.float64) for a in np.mgrid[0:H, 0:W])
    d = depth.reshape(-1).astype(np.float64)
    X = [d * ((Kinv[r, 0] * x + Kinv[r, 1] * y) + Kinv[r, 2] * 1.0) for r in range(3)]
    P = [((cam[r, 0] * X[0] + cam[r, 1] * X[1]) + cam[r, 2] * X[2]) + cam[r, 3] for r in range(3)]
    valid = (depth > 0) & (depth.astype(np.float64) < threshold)
    if mask is not None:
        valid &= np.asarray(mask) == 0
    return np.stack(P, axis=1), valid.reshape(-1)


def project(depth, K, cam, q):
    """orc_depth_sdf's visibility test term for term at q (n, 3): pc_z, ux, uy (camera depth and pixel coordinates), in_view
    (the truncated pixel lies in the image), d_pix (the image's depth there, 0 where not in view), inside."""
    H, W = depth.shape
    ci = np.linalg.inv(cam)
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    pc = [((ci[r, 0] * q[:, 0] + ci[r, 1] * q[:, 1]) + ci[r, 2] * q[:, 2]) + ci[r, 3] for r in range(3)]
    u = [(K[r, 0] * pc[0] + K[r, 1] * pc[1]) + K[r, 2] * pc[2] for r in range(3)]
    with np.errstate(all="ignore"):
        ux, uy = u[0] / u[2], u[1] / u[2]
        fx, fy = np.abs(ux) < 9.0e18, np.abs(uy) < 9.0e18  # false for NaN
    ix = np.where(fx, np.trunc(np.where(fx, ux, 0.0)), -1.0).astype(np.int64)
    iy = np.where(fy, np.trunc(np.where(fy, uy, 0.0)), -1.0).astype(np.int64)
    in_view = (ix >= 0) & (iy >= 0) & (ix < W) & (iy < H)
    d_pix = np.where(in_view, depth[np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)].astype(np.float64), 0.0)
    inside = in_view & ~(pc[2] < d_pix)
    return SimpleNamespace(pc_z=pc[2], ux=ux, uy=uy, ix=ix, iy=iy, in_view=in_view, d_pix=d_pix, inside=inside)


def undecided(depth, K, cam, q, tol=1e-9):
    """Points whose side of the visibility test a change of `tol` in camera depth or pixel coordinates could turn: the
    camera depth within tol of the image's at the pixel, or a pixel coordinate within tol of an integer (every value at
    which truncation changes the pixel or leaves the image is one)."""
    p = project(depth, K, cam, q)
    with np.errstate(all="ignore"):
        near = lambda a: ~(np.abs(a - np.rint(a)) >= tol)  # NaN and inf count as near
        return (p.in_view & (np.abs(p.pc_z - p.d_pix) < tol)) | near(p.ux) | near(p.uy)


# ------------------------------------------------------------------------------------------ cameras
def tilted_camera(a, xyz):
    """Looking along +x of the world and down by the angle a."""
    cam = np.eye(4)
    cam[:3, :3] = np.array([[0, -np.sin(a), np.cos(a)], [-1.0, 0, 0], [0, -np.cos(a), -np.sin(a)]])
    cam[:3, 3] = xyz
    return cam


def intrinsics(H, W, skew=0.0):
    f = 0.9 * max(H, W) + 3.0  # the longer side spans about 58 degrees
    return np.array([[f, skew, W / 2.0 + 0.21], [0, 0.985 * f, H / 2.0 + 0.13], [0, 0, 1.0]])


# ------------------------------------------------------------------------------------------ images
_SPECS = [  # name, H, W, nq
    ("one_pixel", 1, 1, 65), ("one_tile", 4, 8, 1), ("under_tile", 3, 5, 63), ("tile_plus_one", 5, 9, 64),
    ("row_strip", 1, 200, 255), ("col_strip", 130, 1, 257), ("pow2_full", 32, 64, 256), ("pow2_over", 33, 65, 3000),
    ("widest_tree", 1, 8192, 2000), ("past_the_tree", 1, 8200, 1500), ("single_valid", 33, 65, 257),
    ("none_valid", 12, 20, 65), ("holes", 33, 65, 1000), ("flat_wall", 20, 40, 256)]
STATED_P = dict(one_pixel=1, one_tile=1, under_tile=1, tile_plus_one=2, row_strip=32, col_strip=64, pow2_full=8, pow2_over=16,
                widest_tree=1024, past_the_tree=2048, single_valid=16, none_valid=4, holes=16, flat_wall=8)
SINGLE_PIXEL = (18, 43)  # the valid pixel of single_valid (row, column)
THRESHOLD = 1.5


def _image(name, H, W, rng):
    """depth (float32), mask or None, K, cam of a case."""
    depth = (0.6 + 0.5 * rng.random((H, W))).astype(np.float32)
    mask = None
    K = intrinsics(H, W, skew=0.3 if name in ("pow2_over", "holes", "under_tile") else 0.0)
    cam = tilted_camera(0.3, [-0.3, 0.1, 0.8])
    if name in ("under_tile", "tile_plus_one"):
        depth[H - 1, 1] = 0.0
    elif name in ("row_strip", "col_strip", "pow2_full", "pow2_over", "widest_tree", "past_the_tree"):
        depth[rng.random((H, W)) < 0.1] = 0.0
        if name in ("pow2_over", "col_strip", "widest_tree"):
            mask = (rng.random((H, W)) < 0.05).astype(np.uint8)
        depth[H - 1, W - 1] = np.float32(0.9)  # the last pixel of the last tile counts
        if mask is not None:
            mask[H - 1, W - 1] = 0
    elif name == "single_valid":  # (no mask: the first cloud of gto_scene_from_depth ignores it)
        depth[:, :32] = 0.0
        depth[:, 32:] = 2.0
        for _ in range(64):  # a depth at which the point's own projection, rounded, still counts as inside: -0.0
            depth[SINGLE_PIXEL] = np.float32(rng.uniform(0.6, 1.1))
            pts, valid = backproject(depth, K, cam, None, THRESHOLD)
            if project(depth, K, cam, pts[valid]).inside.all():
                break
        else:
            raise AssertionError("single_valid: no depth puts the point's own projection inside")
    elif name == "none_valid":
        depth[:, :7] = 0.0
        depth[:, 7:14] = 2.0
        mask = np.zeros((H, W), np.uint8)
        mask[:, 14:] = 1
    elif name == "holes":
        mask = np.zeros((H, W), np.uint8)
        for cy, cx in ((0, 0), (1, 1), (2, 5), (3, 3), (4, 3), (4, 4), (5, 3), (5, 4), (8, 8), (7, 0)):  # dead tiles
            depth[4 * cy:4 * cy + 4, 8 * cx:8 * cx + 8] = 0.0
        depth[18, 27] = np.float32(0.8)  # one live pixel in the block of four dead tiles (rows 16-23, columns 24-39)
        for cy, cx in ((0, 2), (2, 6), (6, 1), (6, 2), (8, 0)):  # masked tiles
            mask[4 * cy:4 * cy + 4, 8 * cx:8 * cx + 8] = 1
        depth[:, 52:55] = 2.0  # a stripe beyond the threshold
    elif name == "flat_wall":
        depth[:] = np.float32(0.875)
        cam = np.eye(4)
        cam[:3, 3] = [0.25, -0.125, 0.5]
    return depth, mask, K, cam


def _queries(name, depth, mask, K, cam, nq, rng):
    """(query (nq, 3), on_cloud: the indices of the queries that are cloud points)."""
    H, W = depth.shape
    pts, valid = backproject(depth, K, cam, mask, THRESHOLD)
    cloud = pts[valid]
    n_on = min(len(cloud), max(1, nq // 8))
    n_far = min(4, nq // 16)
    n_z0 = 8 if name == "flat_wall" else 0
    n_edge = (nq - n_on - n_far - n_z0) // 3
    n_box = nq - n_on - n_far - n_z0 - n_edge
    on = np.zeros((0, 3))
    if n_on:  # a cloud point's own camera depth and pixel come back rounded: which side it falls on varies; take of both
        ins = project(depth, K, cam, cloud).inside
        first = rng.permutation(np.flatnonzero(ins))[:(n_on + 1) // 2]
        rest = rng.permutation(np.setdiff1d(np.arange(len(cloud)), first))
        on = cloud[np.concatenate([first, rest])[:n_on]]
    far = np.array([[1.0e6, 0.0, 0.0], [-1.0e6, 1.0e6, 0.7], [0.3, 0.1, -1.0e6], [3.0e5, -1.0e6, 1.0e6]])[:n_far]
    z0 = np.concatenate([rng.uniform(-1.0, 1.0, (n_z0, 2)), np.full((n_z0, 1), cam[2, 3])], axis=1)
    if n_z0:
        z0[0] = cam[:3, 3]  # the camera centre itself: 0 / 0
    # through pixel coordinates: half of them in (-1, 0), depths from in front of the surfaces to behind them
    zc = rng.uniform(0.3, 1.6, n_edge)
    u = np.where(rng.random(n_edge) < 0.5, rng.uniform(-1.0, 0.0, n_edge), rng.uniform(0.0, W, n_edge))
    v = np.where(rng.random(n_edge) < 0.5, rng.uniform(-1.0, 0.0, n_edge), rng.uniform(0.0, H, n_edge))
    edge = (np.linalg.inv(K) @ np.stack([u * zc, v * zc, zc])).T @ cam[:3, :3].T + cam[:3, 3]
    # two boxes: the cloud's grown by 0.15 m, and by 1.2 m (the camera is at most 1.1 m from any of its points)
    lo, hi = (cloud.min(0), cloud.max(0)) if len(cloud) else (cam[:3, 3] - 0.3, cam[:3, 3] + 0.3)
    n_wide = n_box // 2
    box = np.concatenate([rng.uniform(lo - 0.15, hi + 0.15, (n_box - n_wide, 3)), rng.uniform(lo - 1.2, hi + 1.2, (n_wide, 3))])
    q = np.concatenate([on, far, z0, edge, box])
    order = rng.permutation(nq)
    return np.ascontiguousarray(q[order]), np.flatnonzero(order < n_on)


_CASES = None


def cases():
    """{name: case}; a case has name, depth (float32 H x W), K, cam, mask (uint8 or None), threshold, query (nq, 3), epsilon,
    w_inside, P, and on_cloud / neg_zero: the queries that are cloud points / those of them the visibility test puts inside."""
    global _CASES
    if _CASES is None:
        _CASES = {}
        for k, (name, H, W, nq) in enumerate(_SPECS):
            rng = np.random.default_rng(4100 + k)
            depth, mask, K, cam = _image(name, H, W, rng)
            query, on_cloud = _queries(name, depth, mask, K, cam, nq, rng)
            neg_zero = on_cloud[project(depth, K, cam, query[on_cloud]).inside]
            for a in (depth, K, cam, query) + (() if mask is None else (mask,)):
                a.setflags(write=False)
            _CASES[name] = SimpleNamespace(name=name, depth=depth, K=K, cam=cam, mask=mask, threshold=THRESHOLD, query=query,
                                           epsilon=(0.03, 0.05, 0.02)[k % 3], w_inside=(2.0, 1.0, 1.5)[k % 3],
                                           P=tile_levels(H, W), on_cloud=on_cloud, neg_zero=neg_zero)
    return _CASES


# ------------------------------------------------------------------------------------------ workspace grids (cost-only search)
SCENE_NAMES = ["one_pixel", "one_tile", "under_tile", "tile_plus_one", "row_strip", "col_strip", "pow2_full", "pow2_over",
               "single_valid", "holes", "flat_wall"]
BOUNDARY_NAMES = ["single_valid", "flat_wall"]
MAX_VOXELS = 40000


def midpoint_res(near=0.05):
    """A grid resolution (double) exactly half way between two neighbouring float32 values fa < fb near `near`, fb the one
    with the even mantissa: float32(res) == fb (ties to even), and a float64 distance of res (1 +- a few 1e-16) becomes fa or
    fb as its last bits fall, so with epsilon == res the comparison `dist < epsilon` is decided by rounding alone."""
    fa = np.float32(near)
    if fa.view(np.uint32) & 1 == 0:
        fa = np.nextafter(fa, np.float32(1.0))
    fb = np.nextafter(fa, np.float32(1.0))
    res = (float(fa) + float(fb)) / 2.0
    assert np.float32(res) == fb and float(fa) < res < float(fb)
    return res


def target_of(case):
    """A target mask for the second cloud of gto_scene_from_depth: a rectangle in the middle of the image (for a one-pixel
    image: nothing), never the only valid pixel of single_valid."""
    H, W = case.depth.shape
    m = np.zeros((H, W), np.uint8)
    if H * W > 1:
        m[H // 3:max(H // 3 + 1, 2 * H // 3), W // 3:max(W // 3 + 1, 2 * W // 3)] = 1
    if case.name == "single_valid":
        m[SINGLE_PIXEL] = 0
    return m


def voxel_centres(bounds, margin, res):
    """The voxel centres of the grid around bounds (3, 2), C order (gto/gto_models.py:155-171)."""
    axes = [np.arange(bounds[a, 0] - margin, bounds[a, 1] + margin, res) for a in range(3)]
    return np.array(np.meshgrid(*axes, indexing="ij")).reshape((3, -1)).T, tuple(len(a) for a in axes)


def cloud_bounds(case):
    """(3, 2) bounding box of the first cloud of gto_scene_from_depth (every valid pixel, no mask)."""
    pts, valid = backproject(case.depth, case.K, case.cam, None, case.threshold)
    return np.stack([pts[valid].min(0), pts[valid].max(0)], axis=1)


def scene_cases():
    """Grids for gto_scene_from_depth around the small cases: name, case, grid_res, margin, epsilon, w_inside, target (mask),
    depth_obstacle (the driver's copy of the image with the target's pixels at the threshold), boundary.  The ordinary ones
    have a margin of 0.1 m at the resolution (a multiple of 5 mm, at least 4 cm) that keeps the grid under MAX_VOXELS and
    epsilon = 0.06 m, more than a voxel.  The two boundary scenes have epsilon == grid_res == midpoint_res() and a margin
    of three voxels: the centres of index 2 and 4 along an axis are res away from the lowest point of the cloud."""
    out = []
    for name in SCENE_NAMES + [n + "_boundary" for n in BOUNDARY_NAMES]:
        boundary = name.endswith("_boundary")
        case = cases()[name[:-len("_boundary")] if boundary else name]
        ext = np.diff(cloud_bounds(case), axis=1).reshape(3)
        if boundary:
            res = midpoint_res()
            margin, epsilon = 3 * res, res
        else:
            margin, epsilon, res = 0.1, 0.06, 0.04
            while np.prod(np.ceil((ext + 2 * margin) / res) + 1) > MAX_VOXELS:
                res += 0.005
        target = target_of(case)
        dobs = case.depth.copy()
        dobs[target.astype(bool)] = case.threshold
        out.append(SimpleNamespace(name=name, case=case, grid_res=float(res), margin=float(margin), epsilon=float(epsilon),
                                   w_inside=1.5, target=target, depth_obstacle=dobs, boundary=boundary))
    return out


# ------------------------------------------------------------------------------------------ gripper points and poses
POSED_POINTS = [1, 63, 64, 65, 256, 257]


def posed_instance(case, n_points, n_poses=6):
    """Gripper points (n_points, 3) around the origin and poses (n_poses, 4, 4) that put them around the case's queries: a
    small turn about a random axis and a shift to one of the queries (none of those at 1e6 m).  Pose 2 holds a NaN."""
    rng = np.random.default_rng(n_points)
    pts = rng.uniform(-0.08, 0.08, (n_points, 3))
    finite = np.abs(case.query).max(axis=1) < 1.0e5
    inside = np.flatnonzero(project(case.depth, case.K, case.cam, case.query).inside & finite)
    RT = np.tile(np.eye(4), (n_poses, 1, 1))
    for i in range(n_poses):
        w = rng.standard_normal(3)
        w /= np.linalg.norm(w)
        a = rng.uniform(-0.6, 0.6)
        Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        RT[i, :3, :3] = np.eye(3) + np.sin(a) * Wx + (1 - np.cos(a)) * Wx @ Wx
        # every other pose at a query behind a surface, so that some of its points count and some do not
        pick = inside if (i % 2 == 0 and len(inside)) else np.flatnonzero(finite)
        RT[i, :3, 3] = case.query[pick[rng.integers(len(pick))]]
    RT[2, 1, 3] = np.nan
    return pts, RT


def placed(points, poses):
    """World points (n, P, 3) as utils.grasp_collision_ratio places them."""
    return np.einsum("nij,pj->npi", poses[:, :3, :3], points) + poses[:, None, :3, 3]


# ------------------------------------------------------------------------------------------ plans through an image
PLAN_ROBOTS = ["panda", "random", "bushy8", "chain16"]
PLAN_HORIZONS = [5, 7, 22, 50, 96]  # T % 4 = 1, 3, 2, 2, 0: k_check_plans takes four waypoints per workgroup
PLAN_B = 3


def plan_robot(name):
    """(desc, link_ee, link_gripper, n_gripper_points) of a robot of PLAN_ROBOTS."""
    from helpers import cfg_of, limit_robot, random_robot
    from grasptrajopt_amd.robot_desc import load_builtin
    if name == "panda":
        cfg = cfg_of("panda")
        return load_builtin("panda"), cfg["link_ee"], cfg["link_gripper"], None
    if name == "random":
        desc, ee = random_robot(3)  # 21 frames, prismatic joints among the optimised and the parameter joints
    else:
        desc, ee = limit_robot({"bushy8": "bushy", "chain16": "chain"}[name], n_opt={"bushy8": 8, "chain16": 16}[name])
    return desc, ee, ee, 40


def plan_instance(name, desc, T, world_points, seed=0, key=None):
    """B = 3 straight joint-space plans of `desc` over T waypoints and a depth image they reach through.
    world_points(q (n, ndof), base (n, 3)) -> (n, P, 3): the robot's surface points in the world (the oracle's).
    The camera stands behind the robot and looks along +x.  The image hugs the first half of the motion from behind: a
    pixel's depth is that of the farthest point the waypoints t <= (T - 1) / 2 put there (with the shared base and with
    the per-plan bases) plus 1 to 1.4 cm, so these waypoints count 0; a pixel none of them reaches lies in front of the
    whole robot, so what the second half of the motion moves there counts.  No two pixels are alike.  Returns plans
    (B, ndof, T), base (3,), bases (B, 3), nan_at (plan, joint, waypoint), depth, K, cam.  A robot outside PLAN_ROBOTS
    (tests/small_robots.py) gives the `key` that stands for its place in that list."""
    rng = np.random.default_rng(7000 + 100 * (PLAN_ROBOTS.index(name) if key is None else key) + T + 1000 * seed)
    B = PLAN_B
    if name == "panda":
        from helpers import cfg_of
        q0 = np.array(cfg_of("panda")["default_pose"], dtype=np.float64)
    else:
        q0 = rng.uniform(0.3 * desc.lower, 0.3 * desc.upper)
    opt = np.asarray(desc.opt_index)
    plans = np.tile(q0[None, :, None], (B, 1, T))
    for b in range(B):
        qg = rng.uniform(0.8 * desc.lower[opt], 0.8 * desc.upper[opt])
        plans[b, opt, :] = q0[opt, None] + (qg - q0[opt])[:, None] * np.linspace(0.0, 1.0, T)[None, :]
    base = rng.uniform(-0.05, 0.05, 3)
    bases = rng.uniform(-0.08, 0.08, (B, 3))
    q = plans.transpose(0, 2, 1).reshape(B * T, desc.ndof)
    xyz = np.stack([world_points(q, np.tile(base, (B * T, 1))), world_points(q, np.repeat(bases, T, axis=0))]).reshape(2, B, T, -1, 3)
    lo, hi = xyz.reshape(-1, 3).min(0), xyz.reshape(-1, 3).max(0)
    c = (lo + hi) / 2
    e_lat = max(hi[1] - lo[1], hi[2] - lo[2]) / 2
    D = 1.0 + 2 * e_lat  # from the camera to the nearest point
    H, W = 60, 80
    f = (H / 2) * D / (1.3 * e_lat)
    K = np.array([[f, 0, W / 2 + 0.37], [0, f, H / 2 + 0.21], [0, 0, 1.0]])
    cam = tilted_camera(0.0, [lo[0] - D, c[1], c[2]])
    first = xyz[:, :, :(T - 1) // 2 + 1].reshape(-1, 3)
    p = project(np.zeros((H, W), np.float32), K, cam, first)
    assert p.in_view.all()
    zmax = np.full((H, W), -np.inf)
    np.maximum.at(zmax, (p.iy, p.ix), p.pc_z)
    depth = np.where(zmax > -np.inf, zmax + 0.01, D - 0.05) + rng.uniform(0.0, 0.004, (H, W))
    depth = depth.astype(np.float32)
    nan_at = (1, int(opt[len(opt) // 2]), T // 2)
    return SimpleNamespace(name=name, T=T, plans=plans, base=base, bases=bases, nan_at=nan_at, depth=depth, K=K, cam=cam,
                           threshold=float(depth.max()) + 1.0)


def plan_expected(inst, desc, world_points, bases):
    """(counts (B, T) int32 with -1 at the NaN waypoint, number of undecided points) for the plans of `inst` with the NaN
    planted, at bases (3,) or (B, 3): the oracle's points through the visibility test."""
    B, T = PLAN_B, inst.T
    b3 = np.broadcast_to(np.asarray(bases, dtype=np.float64).reshape(-1, 3), (B, 3))
    q = inst.plans.transpose(0, 2, 1).reshape(B * T, desc.ndof)
    xyz = world_points(q, np.repeat(b3, T, axis=0)).reshape(-1, 3)
    inside = project(inst.depth, inst.K, inst.cam, xyz).inside.reshape(B, T, -1)
    und = undecided(inst.depth, inst.K, inst.cam, xyz).reshape(B, T, -1)
    counts = inside.sum(axis=2).astype(np.int32)
    p, _, t = inst.nan_at
    counts[p, t] = -1
    und[p, t] = False
    return counts, int(und.sum())
