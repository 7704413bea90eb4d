"""Numpy restatement of the stream-ordered base placement (gto_occupancy_*, gto_base_report_device; include/gto_solver.h) and
the cases tests/test_base_chain_cpu.py and tests/test_gpu_base_chain.py share.

The occupancy grid is GTORobotModel.setup_occupancy_grid itself, called unbound on a namespace as
tests/test_oracle_golden.py does (it is pinned on the reference there).  The report follows gto/base_planner.py:127-162 with
the FP64 oracle's kinematics.  The collision count is a sum of grid lookups at floor((p - origin) / resolution): a kernel and
this restatement agree on it exactly when no placed point lies within round-off of a cell edge, which `clearance` measures and
every case asserts (CLEARANCE; the kinematics of the two sides differ by 1e-15 m, the placed points by a few times that)."""
import types

import numpy as np

from grasptrajopt_amd.gto_models import GTORobotModel
from grasptrajopt_amd.robot_desc import load_builtin
from helpers import cfg_of, limit_robot, random_robot

MARGIN, RES, EPS = 0.4, 0.05, 0.02
CLEARANCE = 1e-9


# ------------------------------------------------------------------------------------------------- the grid
def grid(points, margin=MARGIN, res=RES, epsilon=EPS):
    """The attributes GTORobotModel.setup_occupancy_grid fills, on a namespace."""
    o = types.SimpleNamespace(field_margin=margin, grid_resolution=res)
    with np.errstate(invalid="ignore"):  # (rint of an infinite coordinate: numpy casts it to the smallest integer, off the grid)
        GTORobotModel.setup_occupancy_grid(o, np.asarray(points, dtype=np.float64), epsilon)
    return o


def offsets(g, pts):
    return GTORobotModel.points_to_offsets_occupancy_numpy(g, pts)


def grid_points(n, seed, margin=MARGIN, res=RES, epsilon=EPS):
    """n points that exercise k_occ_mark: a random cloud over a few grid cells' worth of table, points at and below the height
    cut, points so far behind x = 0 that their nodes fall off the grid, points on nodes and at node +- epsilon, a point with
    NaN height and one at x = -inf (numpy keeps both out of the grid)."""
    rng = np.random.default_rng(seed)
    p = np.c_[rng.uniform(0.0, 1.3, n), rng.uniform(-0.7, 0.9, n), rng.uniform(0.02, 0.8, n)]
    p[0] = [1.3, 0.9, 0.5]   # the bounds do not move with the edits below
    if n > 1:
        p[1] = [0.6, -0.7, 0.5]
    k = np.arange(2, n)
    low, off, node, edge = k[k % 11 == 0], k[k % 11 == 1], k[k % 11 == 2], k[k % 11 == 3]
    p[low, 2] = np.where(np.arange(len(low)) % 2 == 0, 0.01, rng.uniform(-0.2, 0.01, len(low)))
    p[off, 0] = -margin - epsilon - rng.uniform(1e-3, 0.5, len(off))
    if len(node) or len(edge):
        xg = np.arange(0.0 - margin, 1.3 + margin, res)  # the axes the bounds above give
        yg = np.arange(-0.7 - margin, 0.9 + margin, res)
        for idx, d in ((node, 0.0), (edge, epsilon)):
            ix, iy = rng.integers(0, len(xg), len(idx)), rng.integers(0, len(yg), len(idx))
            sgn = np.where(np.arange(len(idx)) % 2 == 0, 1.0, -1.0)
            p[idx, 0] = np.clip(xg[ix] + sgn * d, None, 1.3)
            p[idx, 1] = np.clip(yg[iy], -0.7, 0.9)
    if n > 40:
        p[5] = [0.5, 0.1, np.nan]
        p[6] = [-np.inf, 0.2, 0.4]
    return p


# ------------------------------------------------------------------------------------------------- the report
def base_matrix(y):
    c, s = np.cos(y[2]), np.sin(y[2])
    return np.array([[c, -s, 0, y[0]], [s, c, 0, y[1]], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])


def report(orc, fe, fg, goals, n_goals, y, q, fill=np.nan):
    """err_pos, err_rot (B, n_max) of gto/base_planner.py:130-144; rows >= n_goals[b] hold `fill`."""
    B, n_max = goals.shape[:2]
    fr = orc.eval_fk(q.reshape(B * n_max, -1)).reshape(B, n_max, -1, 4, 4)
    ep, er = np.full((B, n_max), fill), np.full((B, n_max), fill)
    for b in range(B):
        Bm = base_matrix(y[b])
        for i in range(int(n_goals[b])):
            Tg = fr[b, i, fg]
            RT = Bm @ goals[b, i].reshape(4, 4) @ (np.linalg.inv(fr[b, i, fe]) @ Tg)
            ep[b, i] = np.linalg.norm(RT[:3, 3] - Tg[:3, 3])
            er[b, i] = np.degrees(np.arccos(np.clip((np.trace(RT[:3, :3].T @ Tg[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))
    return ep, er


def footprint(orc, qc):
    """The robot's surface points at qc (B, ndof) with a zero base, (B, P, 3)."""
    return orc.eval_points(0, qc, [0.0, 0.0, 0.0], want_field=False)[0]


def place(pts, y):
    """Surface points in the frame of the new base: the formulas of gto_base_report_device."""
    c, s = np.cos(y[2]), np.sin(y[2])
    dx, dy = pts[:, 0] - y[0], pts[:, 1] - y[1]
    return np.c_[c * dx + s * dy, -s * dx + c * dy, pts[:, 2]]


def place_by_inverse(pts, y):
    """BasePlanner.base_collision_cost's formulation: np.linalg.inv of the base matrix as tf_base."""
    M = np.linalg.inv(base_matrix(y))
    return pts @ M[:3, :3].T + M[:3, 3]


def collision(g, placed):
    return int(np.sum(g.occupancy_grid[offsets(g, placed)]))


def collisions(g, foot, y, qc):
    """collision_out: -1 for a set whose y or qc has a non-finite entry."""
    return np.array([collision(g, place(foot[b], y[b])) if np.isfinite(y[b]).all() and np.isfinite(qc[b]).all() else -1
                     for b in range(len(y))], dtype=np.int32)


def clearance(g, placed):
    """The smallest distance of a placed point to a cell edge in x or y (points more than a cell outside the grid are
    clipped to its border whatever their round-off)."""
    u = (placed[:, :2] - g.occupancy_grid_origin) / g.grid_resolution
    n = np.asarray(g.occupancy_grid_shape, dtype=np.float64)
    near = (u > -1.0) & (u < n + 1.0)
    d = np.abs(u - np.rint(u))[near]
    return float(d.min() * g.grid_resolution) if d.size else np.inf


def first_free(coll):
    free = np.flatnonzero(np.asarray(coll) == 0)
    return int(free[0]) if len(free) else -1


FIRST_FREE_PATTERNS = {  # name -> (B, indices of the free sets, indices of the sets marked -1)
    "none": (130, [], []), "only0": (130, [0], []), "last": (130, [129], []), "at63": (130, [63, 100], []),
    "at64": (130, [64, 65], []), "at65": (130, [65], []), "bad_before": (130, [70], [0, 3, 64, 69]), "one": (1, [0], []),
}


def first_free_pattern(name):
    B, free, bad = FIRST_FREE_PATTERNS[name]
    coll = np.arange(1, B + 1, dtype=np.int32)
    coll[free], coll[bad] = 0, -1
    return coll


def first_free_scene(orc, pattern):
    """The scene of a first-free pattern on Fetch: sets that stand in a densely observed patch collide; a set whose base moves
    five metres away sees every point clipped to the grid's border, which the margin keeps free; a NaN marks a set -1.
    Asserts the clearance of every finite set and that the restated counts make the pattern."""
    B, free, bad = FIRST_FREE_PATTERNS[pattern]
    qc = np.tile(np.array(cfg_of("fetch")["default_pose"], dtype=np.float64), (B, 1))
    xs, ys = np.meshgrid(np.arange(0.0, 0.6, 0.02), np.arange(-0.4, 0.4, 0.02), indexing="ij")
    cloud = np.c_[xs.ravel() + 0.003, ys.ravel() + 0.003, np.full(xs.size, 0.5)]
    y = np.tile([0.013, -0.021, 0.1], (B, 1))
    y[free] = [-5.0, 0.0, 0.0]
    y[bad, 1] = np.nan
    g = grid(cloud)
    foot = footprint(orc, qc[:1])[0]
    for b in range(B):
        if b not in bad:
            c = clearance(g, place(foot, y[b]))
            assert c >= CLEARANCE, (b, c)
    want = collisions(g, np.broadcast_to(foot, (B,) + foot.shape), y, qc)
    assert [int(b) for b in np.flatnonzero(want == 0)] == sorted(free) and [int(b) for b in np.flatnonzero(want == -1)] == sorted(bad)
    return types.SimpleNamespace(qc=qc, y=y, q=qc[:, None].copy(), goals=np.tile(np.eye(4).reshape(1, 1, 16), (B, 1, 1)),
                                 n_goals=np.ones(B, np.int32), cloud=cloud, grid=g, want=want)


# ------------------------------------------------------------------------------------------------- robots and cases
def robot(name):
    """(desc, link_ee, link_gripper, gripper points of the handle) of a test robot."""
    if name in ("fetch", "panda"):
        cfg = cfg_of(name)
        return load_builtin(name), cfg["link_ee"], cfg["link_gripper"], None
    desc, ee = limit_robot("bushy", n_opt=8) if name == "bushy" else random_robot(int(name))
    return desc, ee, ee, 40


REPORT_CASES = [("fetch", 1, 1, 0), ("fetch", 65, 10, 1), ("fetch", 130, 32, 2), ("panda", 65, 2, 3), ("panda", 130, 10, 4),
                ("3", 65, 32, 5), ("3", 1, 2, 6), ("bushy", 130, 10, 7), ("bushy", 65, 1, 8)]


def report_case(orc, desc, B, n_max, seed):
    """Random in-limit configurations, random base poses and goal poses (any rigid transforms: the report needs no solve),
    ragged goal counts, and an observed cloud around the robot dense enough that most footprints meet occupied nodes.
    Asserts the clearance of every set."""
    rng = np.random.default_rng(1000 + seed)
    ndof = desc.ndof
    qc = rng.uniform(0.8 * desc.lower, 0.8 * desc.upper, (B, ndof))
    q = rng.uniform(0.8 * desc.lower, 0.8 * desc.upper, (B, n_max, ndof))
    y = np.c_[rng.uniform(-0.3, 0.3, (B, 2)), rng.uniform(-np.pi, np.pi, B)]
    goals = np.tile(np.eye(4), (B, n_max, 1, 1))
    for g4 in goals.reshape(-1, 4, 4):
        g4[:3, :3] = base_matrix([0, 0, rng.uniform(-3, 3)])[:3, :3] @ np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]])
        g4[:3, 3] = rng.uniform(-0.8, 0.8, 3)
    n_goals = rng.integers(1, n_max + 1, B).astype(np.int32)
    n_goals[0] = n_max
    foot = footprint(orc, qc)
    span = float(np.abs(foot[..., :2]).max()) + 0.5
    cloud = np.c_[rng.uniform(0.0, span, 600), rng.uniform(-span, span, 600), rng.uniform(0.02, 1.0, 600)]
    g = grid(cloud, epsilon=0.04)
    for b in range(B):
        c = clearance(g, place(foot[b], y[b]))
        assert c >= CLEARANCE, (b, c)
    return types.SimpleNamespace(qc=qc, q=q, y=y, goals=goals.reshape(B, n_max, 16), n_goals=n_goals, cloud=cloud, grid=g, foot=foot,
                                 epsilon=0.04)
