"""The held-clearance statistic of gto_held_clearance restated in numpy, and the cases the CPU and the GPU test file share
(no GPU here).

reference() takes WORLD robot points and the held points already carried to the column, so that the kinematics are whoever
made them: the oracle's on the CPU, h.eval_points' and h.eval_fk's on the GPU, where the library's d2, link and point must
then equal these bit for bit.  The held points go through tests/held_ref.py's place / attach / carry, the three formulas of
gto_check_held_paths, with a ZERO base in carry: Y_t is that header's X_t without the final + base (s + 0.0 is s).  The
squared distance is (dx*dx + dy*dy) + dz*dz, d = Y - X, one rounding per product and per sum."""
import numpy as np

import held_ref as HR
import self_clearance_ref as SR


def carried(E_t, E_a, base, x, pose=None):
    """The held points x (n, 3) (object-frame points with pose (4, 4)) at every column, (Tp, n, 3), at base 0: attached to
    link_ee's frame E_a (4, 4) at the grasp, where the robot stands at ``base``, and carried by the frames E_t (Tp, 4, 4)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    if pose is not None:
        x = HR.place(x, pose)
    return HR.carry(HR.attach(x, np.asarray(base, dtype=np.float64), E_a), E_t, np.zeros(3))


def reference(X, point_link, links, Y, cutoff=np.inf):
    """(d2, link, point) of one column: the robot's world points X (P, 3), their links (P,), the enabled links (L,) bool,
    the carried held points Y (n, 3) and the cutoff in metres.  d2 = min(the smallest squared distance between a held point
    with finite coordinates and a point of an enabled link, cutoff^2); link and point are the lexicographically smallest
    (link, held point) that attains it, -1 when nothing is closer than the cutoff.  A non-finite X gives (nan, -1, -1)."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64).reshape(-1, 3)
    if not np.isfinite(X).all():
        return np.nan, -1, -1
    c2 = np.float64(cutoff) * np.float64(cutoff)
    idx = np.nonzero(np.isfinite(Y).all(axis=1))[0]
    best, link, point = np.inf, -1, -1
    for l in np.nonzero(np.asarray(links))[0]:
        G = X[point_link == l]
        if not len(G) or not len(idx):
            continue
        d = Y[idx][:, None, :] - G[None, :, :]
        m = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(axis=1)
        k = int(m.argmin())  # the first: the lowest held point of the link's minimum
        if m[k] < best:  # strict: of equal minima the lowest link stays
            best, link, point = float(m[k]), int(l), int(idx[k])
    if best < c2:
        return best, link, point
    return float(c2), -1, -1


def reference_paths(X, point_link, links, Y, cutoff=np.inf):
    """reference() over robot points X (B, Tp, P, 3) and carried points Y[b] (Tp, n_b, 3): d2 (B, Tp), link and point
    (B, Tp) int32 as the library returns them."""
    B, Tp = X.shape[:2]
    d2, link, point = np.empty((B, Tp)), np.empty((B, Tp), dtype=np.int32), np.empty((B, Tp), dtype=np.int32)
    for b in range(B):
        for t in range(Tp):
            d2[b, t], link[b, t], point[b, t] = reference(X[b, t], point_link, links, Y[b][t], cutoff)
    return d2, link, point


def apply_cutoff(d2_inf, link_inf, point_inf, c):
    """What a call with cutoff c must return, from the result without one: min(d2, c*c), link and point -1 where far."""
    c2 = np.float64(c) * np.float64(c)
    near = d2_inf < c2
    return np.where(near, d2_inf, c2), np.where(near, link_inf, -1).astype(np.int32), np.where(near, point_inf, -1).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ cases
ROBOTS = SR.ROBOTS
BOX_SIZE = (0.21, 0.06, 0.16)  # metres: a cracker box
N_BOX = 256
# The held box in link_ee's frame: the axis its centre lies along and how far.  The columns are draws of
# self_clearance_ref.columns (the seeds of its COLUMN_SEEDS, N_DRAWS draws): the first ten, which are mostly far, and ten that
# drive the box into the arm, picked with the oracle's kinematics (tests/test_held_clearance_cpu.py holds the table to what
# it has to exercise).
HELD = {"panda": dict(link_ee="panda_hand", axis=2, offset=0.10,
                      picks=list(range(10)) + [284, 293, 62, 74, 140, 123, 142, 75, 21, 174],
                      expect=["panda_link%d" % i for i in range(6)]),
        "fetch": dict(link_ee="wrist_roll_link", axis=0, offset=0.17,
                      picks=list(range(10)) + [148, 94, 32, 55, 264, 273, 35, 14, 102, 77],
                      expect=["shoulder_pan_link", "shoulder_lift_link", "upperarm_roll_link", "elbow_flex_link",
                              "forearm_roll_link"])}
# (at least this many of a robot's 20 columns below the clearance, beyond the cutoff, distinct closest links among the near)
MUST_EXERCISE = {"panda": (8, 8, 4), "fetch": (3, 8, 2)}
BASE = np.array([0.03, -0.02, 0.01])  # where the robot stands at the grasp: it cancels, up to the attach step's bits


def box(robot):
    """The box's N_BOX surface samples in link_ee's frame: faces by area in the order -x +x -y +y -z +z, uniform on the face."""
    rng = np.random.default_rng(3)
    sx, sy, sz = BOX_SIZE
    areas = np.array([sy * sz, sy * sz, sx * sz, sx * sz, sx * sy, sx * sy])
    face = rng.choice(6, size=N_BOX, p=areas / areas.sum())
    u = rng.uniform(-0.5, 0.5, (N_BOX, 3))
    u[np.arange(N_BOX), face // 2] = np.where(face % 2 == 0, -0.5, 0.5)
    centre = np.zeros(3)
    centre[HELD[robot]["axis"]] = HELD[robot]["offset"]
    return u * np.array(BOX_SIZE) + centre


def robot_columns(robot, desc):
    """The robot's columns (20, ndof)."""
    return SR.columns(desc, SR.COLUMN_SEEDS[robot], SR.N_DRAWS)[HELD[robot]["picks"]]


def grasp_pose(robot):
    """The configuration the box is grasped at (ndof,): the config's default pose."""
    return np.array(SR.config(robot)["default_pose"], dtype=np.float64)


def held_world(E_a, base, local):
    """World points at the moment of the grasp of points ``local`` (n, 3) given in link_ee's frame E_a (4, 4), the robot
    standing at ``base``: what a caller hands to the library (plain numpy: any bits will do, they are an input)."""
    return local @ E_a[:3, :3].T + E_a[:3, 3] + np.asarray(base)


def link_masks(desc, link_ee):
    """name -> (L,) bool: the planners' default, every link, none, and each default link alone."""
    default = desc.held_links(link_ee)
    out = {"default": default, "all": np.ones(desc.n_links, dtype=bool), "empty": np.zeros(desc.n_links, dtype=bool)}
    for l in np.nonzero(default)[0]:
        only = np.zeros(desc.n_links, dtype=bool)
        only[l] = True
        out["only_" + desc.link_names[l]] = only
    return out
