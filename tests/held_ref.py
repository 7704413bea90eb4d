"""The held object's points along the motion after the grasp (gto_check_held_paths, include/gto_solver.h): a numpy FP64
restatement of its three formulas and the cases of tests/test_held_cpu.py and tests/test_gpu_held.py.  No GPU here.

The restatement works on given link_ee frames (the FP64 oracle's) and is written element by element, one numpy operation per
product and per sum, which numpy does not fuse:
    d[a]   = (x[a] - base[a]) - E_a.tr[a]
    p[c]   = (E_a.R[0][c]*d[0] + E_a.R[1][c]*d[1]) + E_a.R[2][c]*d[2]
    X_t[r] = (((E_t.R[r][0]*p[0] + E_t.R[r][1]*p[1]) + E_t.R[r][2]*p[2]) + E_t.tr[r]) + base[r]
"Inside" is depth_cases.project(...).inside for a depth observation, with the label rule on top (a point that projects to a
pixel whose label is the held object's counts as outside), and cloud_sdf_ref.cloud_sdf(...)["inside"] for a cloud.

A case (one per robot of ROBOTS) is B = 7 plans of TP_FULL = 12 columns that leave one grasp configuration q_att (column 0)
along straight joint-space lines, a blob of P_MAX = 257 points in front of link_ee at q_att, of which plan b holds the first
N_HELD[b], and two observations built from where the oracle's kinematics carry the points:
  depth   a 48 x 64 image (a depth_cases.tilted_camera behind the motion) whose background lies behind everything; the pixels the
          points cover at the grasp show the object's own surface 1 cm in front of the nearest point (label LABEL_OBJECT):
          without labels every held point counts there, with labels none; the pixels every other point of a plan covers at
          the last column show a neighbour 1 cm in front of it (label LABEL_NEIGHBOUR)
  cloud   the jittered closed box of cloud_cases.box_samples across the blob of the last plan at its last column
Lift-like calls take columns 0 .. Tp - 1 with attach NULL; the reverse-like call takes columns 1 .. 11 and names q_att in
plans of T = 12 columns whose last column it is.  Every case reports its decision margin; tests/test_held_cpu.py holds it to
1e-9, four orders above the 1e-13 gto_eval_fk is held to the oracle, so the GPU's counts must be equal.  A case that misses
the margin changes its seed in SEEDS here."""
from types import SimpleNamespace

import numpy as np

import cloud_cases as cc
import cloud_sdf_ref as ref
import depth_cases as dc

ROBOTS = ["panda", "bushy8", "chain16", "panda_renumbered"]
TP_FULL = 12                    # column 0: the grasp; columns 1 .. 11: the motion
TPS = [1, 4, 5, 11]             # one column, a full group, a tail group of one, the lift's length
N_HELD = [0, 1, 63, 64, 65, 256, 257]
B, P_MAX = len(N_HELD), 257
H, W = 48, 64
LABEL_OBJECT, LABEL_NEIGHBOUR = 7, 3
CLOUD_KS = (1, 11)
TOL = 1e-9
SEEDS = {}                      # robot -> seed of its draw where 0 misses the margin
NAN_POINT = (4, 17)             # (plan, held point) of the non-finite-point test: plan 4 holds 65 points


# ------------------------------------------------------------------------------------------------ the restatement
def place(points, pose):
    """Object-frame points (P, 3) in the world: x = R p + t of pose (4, 4) with gto_observation_check_posed's expression."""
    M, x0, x1, x2 = np.asarray(pose, dtype=np.float64).reshape(4, 4), points[:, 0], points[:, 1], points[:, 2]
    rows = []
    for r in range(3):
        s = M[r, 0] * x0
        s = s + M[r, 2] * x2
        s = s + M[r, 1] * x1
        rows.append(s + M[r, 3])
    return np.stack(rows, axis=1)


def attach(x, base, E_a):
    """World points x (P, 3) in link_ee's frame E_a (4, 4) at the grasp: p (P, 3)."""
    d = []
    for a in range(3):
        t = x[:, a] - base[a]
        d.append(t - E_a[a, 3])
    p = []
    for c in range(3):
        s = E_a[0, c] * d[0]
        s = s + E_a[1, c] * d[1]
        s = s + E_a[2, c] * d[2]
        p.append(s)
    return np.stack(p, axis=1)


def carry(p, E_t, base):
    """p (P, 3) placed by link_ee's frames E_t (Tp, 4, 4): X (Tp, P, 3)."""
    out = np.empty((E_t.shape[0], p.shape[0], 3))
    for t, E in enumerate(E_t):
        for r in range(3):
            s = E[r, 0] * p[:, 0]
            s = s + E[r, 1] * p[:, 1]
            s = s + E[r, 2] * p[:, 2]
            s = s + E[r, 3]
            out[t, :, r] = s + base[r]
    return out


def held_world(E_t, E_a, base, x, pose=None):
    """The three formulas: the held points x (P, 3) (object-frame with pose) at every column, (Tp, P, 3)."""
    base = np.asarray(base, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    if pose is not None:
        x = place(x, pose)
    return carry(attach(x, base, E_a), E_t, base)


def count_depth(X, depth, K, cam, labels=None, label=None):
    """counts (Tp,) of X (Tp, P, 3) inside a depth observation, and the margins (camera depth in metres, pixel coordinates
    in pixels).  Rows with a non-finite coordinate are not counted and have no margin."""
    Tp = X.shape[0]
    ok = np.isfinite(X).all(axis=2)
    counts = np.zeros(Tp, dtype=np.int32)
    mz = mpx = np.inf
    for t in range(Tp):
        q = X[t][ok[t]]
        if not len(q):
            continue
        p = dc.project(depth, K, cam, q)
        inside = p.inside.copy()
        if labels is not None:
            Hh, Ww = depth.shape
            lab = labels[np.clip(p.iy, 0, Hh - 1), np.clip(p.ix, 0, Ww - 1)]
            inside &= ~(p.in_view & (lab == label))
        counts[t] = inside.sum()
        if p.in_view.any():
            mz = min(mz, np.abs(p.pc_z - p.d_pix)[p.in_view].min())
        mpx = min(mpx, np.abs(p.ux - np.rint(p.ux)).min(), np.abs(p.uy - np.rint(p.uy)).min())
    return counts, float(mz), float(mpx)


def count_cloud(X, points, normals, k):
    """counts (Tp,) of X (Tp, P, 3) inside a cloud observation, the smallest gap between the k-th and (k+1)-th distance, and
    the number of queries whose majority a change of TOL could turn (cloud_cases.undecided's two rules)."""
    Tp = X.shape[0]
    ok = np.isfinite(X).all(axis=2)
    counts = np.zeros(Tp, dtype=np.int32)
    gap, turnable = np.inf, 0
    for t in range(Tp):
        q = X[t][ok[t]]
        if not len(q):
            continue
        out = ref.cloud_sdf(points, normals, q, k=k)
        counts[t] = out["inside"].sum()
        d2 = out["d2"]
        if d2.shape[1] > k:
            gap = min(gap, float((np.sqrt(d2[:, k]) - np.sqrt(d2[:, k - 1])).min()))
        votes_only = dict(out, d2=np.concatenate([d2[:, :k], np.full((len(d2), 1), np.inf)], axis=1))
        turnable += int(cc.undecided(votes_only, k, TOL).sum())
    return counts, gap, turnable


# ------------------------------------------------------------------------------------------------ robots and motions
def robot(name):
    """(desc, link_ee, link_gripper, n_gripper_points)."""
    if name == "panda_renumbered":
        import renumbered_robots as rn
        desc, ee, gr, ngp = dc.plan_robot("panda")
        return rn.renumber(desc, rn.CASES["panda"][3], True), ee, gr, ngp
    return dc.plan_robot(name)


def _rotation(rng):
    w = rng.standard_normal(3)
    w /= np.linalg.norm(w)
    a = rng.uniform(0.4, 1.2)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(a) * Wx + (1 - np.cos(a)) * Wx @ Wx


_CASES = {}


def case(oracle_mod, name):
    """The case of a robot (see the module text), built once: desc, ee, gripper, ngp, paths (B, ndof, 12), base (3,),
    frames (B, 12, 4, 4) (the oracle's link_ee frames), held (B, P_MAX, 3) (world points; rows at or beyond n_held are
    zeros), n_held (B,), pose (B, 4, 4) and held_obj (the same points in the object's frame), depth / K / cam / labels /
    threshold, points / normals (the cloud), reverse_plans (B, ndof, 12)."""
    if name in _CASES:
        return _CASES[name]
    desc, ee, gr, ngp = robot(name)
    rng = np.random.default_rng(9100 + 10 * ROBOTS.index(name) + 1000 * SEEDS.get(name, 0))
    if name.startswith("panda"):
        from helpers import cfg_of
        q0 = np.array(cfg_of("panda")["default_pose"], dtype=np.float64)
        if name == "panda_renumbered":
            import renumbered_robots as rn
            q0 = rn.to_new(q0, rn.CASES["panda"][3], 0)
    else:
        q0 = rng.uniform(0.3 * desc.lower, 0.3 * desc.upper)
    opt = np.asarray(desc.opt_index)
    span = desc.upper[opt] - desc.lower[opt]
    paths = np.tile(q0[None, :, None], (B, 1, TP_FULL))
    for b in range(B):
        qg = np.clip(q0[opt] + 0.12 * span * rng.uniform(-1.0, 1.0, len(opt)), desc.lower[opt], desc.upper[opt])
        paths[b, opt, :] = q0[opt, None] + (qg - q0[opt])[:, None] * np.linspace(0.0, 1.0, TP_FULL)[None, :]
    base = rng.uniform(-0.05, 0.05, 3)
    o = oracle_mod.Oracle(desc, ee, gr, oracle_mod.reference_opts(), n_gripper_points=ngp)
    frames = o.eval_fk(paths.transpose(0, 2, 1).reshape(B * TP_FULL, desc.ndof))[:, desc.frame_names.index(ee)]
    frames = np.ascontiguousarray(frames.reshape(B, TP_FULL, 4, 4))
    E_a = frames[0, 0]  # (every plan leaves the same configuration)
    centre = E_a[:3, 3] + base + E_a[:3, :3] @ np.array([0.0, 0.0, 0.06])
    blob = centre + np.clip(rng.standard_normal((P_MAX, 3)) * 0.02, -0.05, 0.05)
    n_held = np.array(N_HELD, dtype=np.int32)
    held = np.zeros((B, P_MAX, 3))
    for b in range(B):
        held[b, :n_held[b]] = blob[:n_held[b]]
    # the same points in an object frame that stands somewhere near them
    pose = np.tile(np.eye(4), (B, 1, 1))
    held_obj = np.zeros_like(held)
    for b in range(B):
        pose[b, :3, :3] = _rotation(rng)
        pose[b, :3, 3] = centre + rng.uniform(-0.03, 0.03, 3)
        held_obj[b, :n_held[b]] = (held[b, :n_held[b]] - pose[b, :3, 3]) @ pose[b, :3, :3]
    X = np.stack([held_world(frames[b], frames[b, 0], base, blob) for b in range(B)])  # every plan with the whole blob
    # ---- the depth observation: a camera behind the motion that looks along +x
    flat = X.reshape(-1, 3)
    lo, hi = flat.min(0), flat.max(0)
    c = (lo + hi) / 2
    e_lat = max(hi[1] - lo[1], hi[2] - lo[2]) / 2 + 0.02
    D = 0.6 + 2 * e_lat
    f = (H / 2) * D / (1.3 * e_lat)
    K = np.array([[f, 0, W / 2 + 0.37], [0, f, H / 2 + 0.21], [0, 0, 1.0]])
    cam = dc.tilted_camera(0.0, [lo[0] - D, c[1], c[2]])
    blank = np.zeros((H, W), np.float32)
    p_all = dc.project(blank, K, cam, flat)
    assert p_all.in_view.all()
    depth = np.full((H, W), p_all.pc_z.max() + 0.3)
    labels = np.zeros((H, W), dtype=np.int32)
    p0 = dc.project(blank, K, cam, X[0, 0])
    for b in range(B):  # the neighbours first: the pixels every other point of plan b covers at the last column
        pl = dc.project(blank, K, cam, X[b, TP_FULL - 1, :max(int(n_held[b]), 2):2])
        near = np.full((H, W), np.inf)
        np.minimum.at(near, (pl.iy, pl.ix), pl.pc_z)
        hit = near < np.inf
        depth[hit] = np.minimum(depth[hit], near[hit] - 0.01)
        labels[hit] = LABEL_NEIGHBOUR
    obj = np.zeros((H, W), bool)
    obj[p0.iy, p0.ix] = True
    depth[obj] = p0.pc_z.min() - 0.01  # the object's own seen surface, in front of every point it holds at the grasp
    labels[obj] = LABEL_OBJECT
    depth = (depth + rng.uniform(0.0, 0.004, (H, W))).astype(np.float32)
    # ---- the cloud observation: a closed box across the blob of the last plan (which holds all of it) at its last column
    mid = X[B - 1, TP_FULL - 1].mean(axis=0) + np.array([0.0, 0.03, 0.0])
    blo, bhi = np.floor((mid - 0.04) / cc.SPACING) * cc.SPACING, np.ceil((mid + 0.04) / cc.SPACING) * cc.SPACING
    points, normals = cc.box_samples(blo, bhi, rng)
    reverse_plans = np.ascontiguousarray(paths[:, :, ::-1])  # q_att is their last column; the reversed stretch is columns 1 .. 11
    s = SimpleNamespace(name=name, desc=desc, ee=ee, gripper=gr, ngp=ngp, paths=paths, base=base, frames=frames, held=held,
                        n_held=n_held, pose=pose, held_obj=held_obj, depth=depth, K=K, cam=cam, labels=labels,
                        threshold=float(depth.max()) + 1.0, points=points, normals=normals, reverse_plans=reverse_plans)
    for a in (paths, frames, held, held_obj, pose, depth, labels, points, normals, reverse_plans):
        a.setflags(write=False)
    _CASES[name] = s
    return s


_EXPECTED = {}


def expected(oracle_mod, name, kind, frame="world", nan_point=False):
    """The counts (B, 12) int32 of a case over all its columns and its margins: kind "depth" (no labels), "labels",
    "cloud1", "cloud11"; frame "world" or "object"; nan_point: held point NAN_POINT holds a NaN.  depth kinds return
    (counts, metres, pixels), cloud kinds (counts, gap, turnable).  Computed once."""
    key = (name, kind, frame, nan_point)
    if key in _EXPECTED:
        return _EXPECTED[key]
    s = case(oracle_mod, name)
    counts = np.zeros((B, TP_FULL), dtype=np.int32)
    m1, m2 = np.inf, 0 if kind.startswith("cloud") else np.inf
    for b in range(B):
        n = int(s.n_held[b])
        x = (s.held_obj if frame == "object" else s.held)[b, :n].copy()
        if nan_point and b == NAN_POINT[0]:
            x[NAN_POINT[1], 1] = np.nan
        X = held_world(s.frames[b], s.frames[b, 0], s.base, x, s.pose[b] if frame == "object" else None)
        if kind.startswith("cloud"):
            cnt, gap, turn = count_cloud(X, s.points, s.normals, int(kind[5:]))
            m1, m2 = min(m1, gap), m2 + turn
        else:
            cnt, mz, mpx = count_depth(X, s.depth, s.K, s.cam, s.labels if kind == "labels" else None, LABEL_OBJECT)
            m1, m2 = min(m1, mz), min(m2, mpx)
        counts[b] = cnt
    counts.setflags(write=False)
    _EXPECTED[key] = (counts, m1, m2)
    return _EXPECTED[key]


KINDS = ("depth", "labels", "cloud1", "cloud11")


# ------------------------------------------------------------------------------------------------ the second launch chain
CHUNK = SimpleNamespace(robot="chain16", Tp=65, P_max=4096, B=64, n_samples=33, k=11, n_small=(200, 257))


def chunk_instance(oracle_mod):
    """64 plans of 65 columns with room for 4096 held points each: Tp * P_max * B = 2^24 + 65 * 4096 queries, of which
    chunk_items(64, 65 * 4096) = 63 plans go into the first launch chain and plan 63 alone into a second.  Plan b is motion
    b % 2 of two; it holds the first 200 (b even) or 257 (b odd) of 4096 points, plan 63 all of them.  The observation is a
    cloud of 33 samples around the points' path.  Returns paths, base, held, n_held, points, normals, counts (64, 65)."""
    c = CHUNK
    assert cc.CHUNK_QUERIES // (c.Tp * c.P_max) == c.B - 1
    desc, ee, gr, ngp = robot(c.robot)
    rng = np.random.default_rng(9900)
    q0 = rng.uniform(0.3 * desc.lower, 0.3 * desc.upper)
    opt = np.asarray(desc.opt_index)
    span = desc.upper[opt] - desc.lower[opt]
    two = np.tile(q0[None, :, None], (2, 1, c.Tp))
    for m in range(2):
        qg = np.clip(q0[opt] + 0.12 * span * rng.uniform(-1.0, 1.0, len(opt)), desc.lower[opt], desc.upper[opt])
        two[m, opt, :] = q0[opt, None] + (qg - q0[opt])[:, None] * np.linspace(0.0, 1.0, c.Tp)[None, :]
    base = rng.uniform(-0.05, 0.05, 3)
    o = oracle_mod.Oracle(desc, ee, gr, oracle_mod.reference_opts(), n_gripper_points=ngp)
    frames = o.eval_fk(two.transpose(0, 2, 1).reshape(2 * c.Tp, desc.ndof))[:, desc.frame_names.index(ee)].reshape(2, c.Tp, 4, 4)
    centre = frames[0, 0, :3, 3] + base
    blob = centre + np.clip(rng.standard_normal((c.P_max, 3)) * 0.02, -0.05, 0.05)
    X = [held_world(frames[m], frames[m, 0], base, blob) for m in range(2)]
    points = X[1][c.Tp // 2].mean(axis=0) + rng.standard_normal((c.n_samples, 3)) * 0.03
    normals = rng.standard_normal((c.n_samples, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    flags = []
    for m in range(2):
        out = ref.cloud_sdf(points, normals, X[m].reshape(-1, 3), k=c.k, chunk=8192)
        assert not cc.undecided(out, c.k, TOL).any()
        flags.append(out["inside"].reshape(c.Tp, c.P_max))
    n_held = np.array([c.n_small[b % 2] for b in range(c.B)], dtype=np.int32)
    n_held[c.B - 1] = c.P_max
    counts = np.stack([flags[b % 2][:, :n_held[b]].sum(axis=1) for b in range(c.B)]).astype(np.int32)
    held = np.zeros((c.B, c.P_max, 3))
    for b in range(c.B):
        held[b, :n_held[b]] = blob[:n_held[b]]
    paths = np.ascontiguousarray(two[np.arange(c.B) % 2])
    return SimpleNamespace(desc=desc, ee=ee, gripper=gr, ngp=ngp, paths=paths, base=base, held=held, n_held=n_held, points=points,
                           normals=normals, counts=counts)
