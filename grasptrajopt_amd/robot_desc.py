"""Flat robot description: the kinematic table + surface points the GTO path consumes.

This is the data the reference assembles from the URDF through ``optas.RobotModel``
(optas/models.py:236-321: joint order, optimised / parameter joints, limits) and
``GTORobotModel`` (gto/gto_models.py:62-101: 100 surface points per collision link, visual
origins).  It is plain arrays so it can cross the C ABI (include/gto_solver.h, gto_robot_desc)
and be committed as a small fixture (JSON + NPZ): the GPU box never sees URDFs or meshes.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

from .mesh import load_mesh, sample_surface
from .urdf import Urdf

JOINT_FIXED, JOINT_REVOLUTE, JOINT_PRISMATIC = 0, 1, 2
_JTYPE = {"fixed": JOINT_FIXED, "revolute": JOINT_REVOLUTE, "continuous": JOINT_REVOLUTE,
          "prismatic": JOINT_PRISMATIC}


def _velocity_limit(v: float) -> float:
    """A URDF velocity limit; 0 (no velocity attribute), >= 1e9 (no <limit> element, urdf.py) -> +inf, no limit."""
    return np.inf if v <= 0.0 or v >= 1e9 else float(v)


def _effort_limit(e: float) -> float:
    """A URDF effort limit; 0 (no effort attribute), >= 1e9 (no <limit> element, urdf.py) -> +inf, no limit."""
    return np.inf if e <= 0.0 or e >= 1e9 else float(e)


def _rpy_matrix(rpy) -> np.ndarray:
    """rotz(yaw) @ roty(pitch) @ rotx(roll) (optas/spatialmath.py:186-211; csrc/gto_device.h rpy2r)."""
    cr, sr, cp, sp, cy, sy = np.cos(rpy[0]), np.sin(rpy[0]), np.cos(rpy[1]), np.sin(rpy[1]), np.cos(rpy[2]), np.sin(rpy[2])
    return (np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
            @ np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]]))


def _sym3(six) -> np.ndarray:
    xx, xy, xz, yy, yz, zz = six
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], dtype=np.float64)


def _six(I) -> np.ndarray:
    return np.array([I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]])


def link_inertial_in_link_frame(link):
    """(mass, com (3,), inertia 3x3 about the com in the LINK frame's axes) of a URDF link: the inertial origin's rpy rotates
    the tensor, which the URDF states in the inertial frame's axes, into the link frame (I_link = R I R^T)."""
    R = _rpy_matrix(link.inertial_rpy)
    return float(link.mass), np.asarray(link.inertial_xyz, dtype=np.float64), R @ _sym3(link.inertia) @ R.T


def lump_inertials(urdf: Urdf, order: Sequence[str]):
    """Per kept frame (the links of `order`) one rigid body: frame_mass (F,), frame_com (F, 3), frame_inertia (F, 6: ixx ixy
    ixz iyy iyz izz about the com, in the frame's axes).  A link that is not kept is welded to its nearest kept ancestor
    with every joint on the way at position 0 (its pose there is the product of the joint origins), and the bodies that
    meet on one frame are merged by the parallel-axis theorem, so that no mass of the URDF is lost."""
    fidx = {n: i for i, n in enumerate(order)}
    F = len(order)
    bodies: List[List] = [[] for _ in range(F)]
    for link in urdf.links:
        m, c, I = link_inertial_in_link_frame(link)
        if not m > 0:
            continue
        cur = link.name
        while cur not in fidx:  # pose of the pruned link in its parent, joint at 0
            j = urdf.parent_joint[cur]
            R = _rpy_matrix(j.rpy)
            c, I = R @ c + np.asarray(j.xyz, dtype=np.float64), R @ I @ R.T
            cur = j.parent
        bodies[fidx[cur]].append((m, c, I))
    mass, com, inertia = np.zeros(F), np.zeros((F, 3)), np.zeros((F, 6))
    for f, bs in enumerate(bodies):
        if not bs:
            continue
        mass[f] = sum(b[0] for b in bs)
        com[f] = sum(b[0] * b[1] for b in bs) / mass[f]
        I = np.zeros((3, 3))
        for m, c, Ib in bs:
            d = c - com[f]
            I += Ib + m * (d @ d * np.eye(3) - np.outer(d, d))
        inertia[f] = _six(I)
    return mass, com, inertia


@dataclass
class RobotDesc:
    name: str
    # kinematic frames (links), parents before children
    frame_names: List[str]
    parent: np.ndarray       # (F,) int32
    joint_type: np.ndarray   # (F,) int32
    q_index: np.ndarray      # (F,) int32, -1 for fixed
    origin_xyz: np.ndarray   # (F,3)
    origin_rpy: np.ndarray   # (F,3)
    axis: np.ndarray         # (F,3)
    # actuated joints in URDF order (optas/models.py:349-354)
    actuated_joint_names: List[str]
    lower: np.ndarray        # (ndof,)
    upper: np.ndarray        # (ndof,)
    opt_index: np.ndarray    # (n_opt,) int32   (optas/models.py:366-386)
    param_index: np.ndarray  # (n_param,) int32 (optas/models.py:388-396)
    # collision links with surface points (gto/gto_models.py:62-80), URDF link order
    link_names: List[str] = field(default_factory=list)
    link_frame: np.ndarray = None   # (L,) int32
    visual_xyz: np.ndarray = None   # (L,3)
    visual_rpy: np.ndarray = None   # (L,3)
    points: np.ndarray = None       # (P,3) float64, visual-mesh frame
    normals: np.ndarray = None      # (P,3)
    point_link: np.ndarray = None   # (P,) int32
    # joint velocity limits (ndof,) from <limit velocity>, +inf = no limit (optas/models.py:497-506); None = not recorded
    velocity: Optional[np.ndarray] = None
    # joint effort limits (ndof,) from <limit effort> (N m, or N for a prismatic joint), +inf = no limit; None = not recorded
    effort: Optional[np.ndarray] = None
    # one rigid body per frame (the link that the frame's joint moves): mass (F,), centre of mass (F, 3) in the frame's
    # coordinates, inertia (F, 6) as ixx ixy ixz iyy iyz izz about the centre of mass in the frame's axes.  None = not recorded
    # (the packaged descriptions): set them with set_link_inertials or build the description from a URDF
    frame_mass: Optional[np.ndarray] = None
    frame_com: Optional[np.ndarray] = None
    frame_inertia: Optional[np.ndarray] = None

    # ------------------------------------------------------------------ properties
    @property
    def ndof(self) -> int:
        return len(self.actuated_joint_names)

    @property
    def n_opt(self) -> int:
        return int(self.opt_index.shape[0])

    @property
    def n_frames(self) -> int:
        return len(self.frame_names)

    @property
    def n_links(self) -> int:
        return len(self.link_names)

    @property
    def n_points(self) -> int:
        return 0 if self.points is None else int(self.points.shape[0])

    def frame_index(self, link_name: str) -> int:
        try:
            return self.frame_names.index(link_name)
        except ValueError:
            raise KeyError(f"link '{link_name}' is not a kinematic frame of this description "
                           f"(frames: {self.frame_names})") from None

    def link_is_moving(self) -> np.ndarray:
        """(L,) bool: True if an optimised joint lies on the chain from the root to the link."""
        opt = set(self.opt_index.tolist())
        moved = np.zeros(self.n_frames, dtype=bool)
        for i in range(self.n_frames):
            p = self.parent[i]
            moved[i] = (p >= 0 and moved[p]) or (self.q_index[i] in opt)
        return moved[self.link_frame]

    @property
    def has_inertials(self) -> bool:
        return self.frame_mass is not None

    def set_link_inertials(self, mass, com, inertia) -> None:
        """Record one rigid body per frame: mass (F,), com (F, 3), inertia (F, 6), as the fields above state them."""
        F = self.n_frames
        mass = np.array(mass, dtype=np.float64).reshape(-1)
        com, inertia = np.array(com, dtype=np.float64).reshape(-1, 3), np.array(inertia, dtype=np.float64).reshape(-1, 6)
        if mass.shape != (F,) or com.shape != (F, 3) or inertia.shape != (F, 6):
            raise ValueError(f"set_link_inertials: mass ({F},), com ({F}, 3) and inertia ({F}, 6) expected")
        self.frame_mass, self.frame_com, self.frame_inertia = mass, com, inertia

    def link_points(self, link_name: str) -> np.ndarray:
        l = self.link_names.index(link_name)
        return self.points[self.point_link == l]

    # ------------------------------------------------------------------ self-clearance (gto_self_clearance)
    def world_points(self, q) -> np.ndarray:
        """(P, 3) surface points in the base frame at the configuration q (ndof,), by a plain numpy forward kinematics
        for HOST-side judgements only (rule (b) of self_pairs, recounts in tools): it agrees with the oracle's and the device's
        kinematics to rounding (1e-12 m, tests/test_self_clearance_cpu.py), NOT bit for bit -- the points the device checks are
        gto_eval_points'."""
        q = np.asarray(q, dtype=np.float64).reshape(self.ndof)
        F = self.n_frames
        R, p = np.zeros((F, 3, 3)), np.zeros((F, 3))
        for f in range(F):
            par = self.parent[f]
            Rp, pp = (R[par], p[par]) if par >= 0 else (np.eye(3), np.zeros(3))
            Ro = _rpy_matrix(self.origin_rpy[f])
            u = self.axis[f] / np.linalg.norm(self.axis[f])
            Rj, t = np.eye(3), np.zeros(3)
            if self.joint_type[f] == JOINT_REVOLUTE:
                K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
                a = q[self.q_index[f]]
                Rj = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
            elif self.joint_type[f] == JOINT_PRISMATIC:
                t = q[self.q_index[f]] * u
            R[f] = Rp @ Ro @ Rj
            p[f] = pp + Rp @ (self.origin_xyz[f] + Ro @ t)
        out = np.empty((self.n_points, 3))
        for l in range(self.n_links):
            f = self.link_frame[l]
            Rv = R[f] @ _rpy_matrix(self.visual_rpy[l])
            tv = p[f] + R[f] @ self.visual_xyz[l]
            sel = self.point_link == l
            out[sel] = self.points[sel] @ Rv.T + tv
        return out

    def point_spacing(self) -> float:
        """The sampling's own length scale, metres: the largest, over the links with at least two points, of the median
        distance from a point to its nearest neighbour on the same link.  Two surfaces closer than this cannot be told
        from two that touch, so it is the default ``clearance`` of the self-clearance check (0 without such a link)."""
        worst = 0.0
        for l in range(self.n_links):
            x = self.points[self.point_link == l]
            if x.shape[0] < 2:
                continue
            d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
            np.fill_diagonal(d2, np.inf)
            worst = max(worst, float(np.median(np.sqrt(d2.min(1)))))
        return worst

    def frame_joints_between(self, fa: int, fb: int) -> int:
        """Non-fixed joints on the tree path between the frames fa and fb."""
        def chain(f):
            out = []
            while f >= 0:
                out.append(int(f))
                f = self.parent[f]
            return out
        ca, cb = chain(fa), chain(fb)
        common = set(ca) & set(cb)
        path = [f for f in ca if f not in common] + [f for f in cb if f not in common]
        return sum(1 for f in path if self.joint_type[f] != JOINT_FIXED)

    def joints_between(self, la: int, lb: int) -> int:
        """Non-fixed joints on the tree path between the frames of links la and lb."""
        return self.frame_joints_between(self.link_frame[la], self.link_frame[lb])

    def self_pairs(self, q_ref=None, clearance=None, ignore=()) -> np.ndarray:
        """(L, L) bool, symmetric with a false diagonal: the link pairs the self-clearance check compares
        (SolverHandle.set_self_pairs).  A pair is enabled unless
          (a) fewer than two non-fixed joints lie on the tree path between the two links' frames (neighbours, links that
              move as one body, hand against finger): such links touch by construction;
          (b) ``q_ref`` is given and the two links' points are closer than ``clearance`` (default: point_spacing()) there:
              what is that close at a pose known to be good says nothing (the planners pass the config's default_pose);
          (c) ``ignore`` names it: pairs of link names."""
        L = self.n_links
        M = np.zeros((L, L), dtype=bool)
        for a in range(L):
            for b in range(a + 1, L):
                M[a, b] = self.joints_between(a, b) >= 2
        if q_ref is not None:
            c = self.point_spacing() if clearance is None else float(clearance)
            X = self.world_points(q_ref)
            for a, b in zip(*np.nonzero(M)):
                xa, xb = X[self.point_link == a], X[self.point_link == b]
                if xa.size and xb.size and ((xa[:, None, :] - xb[None, :, :]) ** 2).sum(-1).min() < c * c:
                    M[a, b] = False
        for na, nb in ignore:
            a, b = self.link_names.index(na), self.link_names.index(nb)
            M[min(a, b), max(a, b)] = False
        return M | M.T

    def held_links(self, link_ee: str, ignore=()) -> np.ndarray:
        """(L,) bool: the collision links a held object is measured against (gto_held_clearance's link_mask).  The object
        rides with the frame ``link_ee``.  A link is enabled unless
          (a) fewer than two non-fixed joints lie on the tree path between its frame and link_ee's frame: hand, fingers and
              the wrist link touch the object by construction (rule (a) of self_pairs);
          (b) ``ignore`` names it."""
        fe = self.frame_index(link_ee)
        out = np.array([self.frame_joints_between(self.link_frame[l], fe) >= 2 for l in range(self.n_links)], dtype=bool)
        for name in ignore:
            out[self.link_names.index(name)] = False
        return out

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_urdf(cls, urdf: Urdf, param_joints: Sequence[str] = (),
                  collision_link_names: Optional[Sequence[str]] = None,
                  extra_links: Sequence[str] = (), model_dir: Optional[str] = None,
                  points_per_link: int = 100, seed: int = 0,
                  keep_all_frames: bool = False) -> "RobotDesc":
        """Frames: the links on the way from the root to a collision link or one of ``extra_links`` (every link with
        ``keep_all_frames``).  The links that are pruned keep their inertia: each pruned subtree is lumped rigidly into its
        nearest kept ancestor with the pruned joints at position 0 (lump_inertials).  ``effort`` holds <limit effort> of
        every actuated joint, +inf where the URDF gives 0 or nothing."""
        actuated = [j.name for j in urdf.joints if j.type != "fixed"]
        for j in urdf.joints:
            if j.type not in _JTYPE:
                raise NotImplementedError(f"{j.type} joints are not supported (optas/models.py:865-866)")
        lower = np.array([urdf.joint_map[j].lower for j in actuated], dtype=np.float64)
        upper = np.array([urdf.joint_map[j].upper for j in actuated], dtype=np.float64)
        velocity = np.array([_velocity_limit(urdf.joint_map[j].velocity) for j in actuated], dtype=np.float64)
        effort = np.array([_effort_limit(urdf.joint_map[j].effort) for j in actuated], dtype=np.float64)
        params = [j for j in actuated if j in set(param_joints)]
        opt_index = np.array([i for i, j in enumerate(actuated) if j not in params], dtype=np.int32)
        param_index = np.array([i for i, j in enumerate(actuated) if j in params], dtype=np.int32)

        # collision links in URDF link order, as the reference's surface_pc_map is keyed
        links = [l for l in urdf.links if l.has_visual and l.visual_mesh is not None
                 and (collision_link_names is None or l.name in collision_link_names)]

        root = urdf.get_root()
        needed = set()
        targets = [l.name for l in links] + list(extra_links)
        if keep_all_frames:
            targets = [l.name for l in urdf.links]
        for name in targets:
            if name not in urdf.link_map:
                raise KeyError(f"link '{name}' does not appear in URDF")
            cur = name
            while True:
                needed.add(cur)
                if cur == root:
                    break
                cur = urdf.parent_joint[cur].parent
        children: Dict[str, List[str]] = {}
        for j in urdf.joints:
            children.setdefault(j.parent, []).append(j.child)
        order: List[str] = []
        stack = [root]
        while stack:  # depth-first, document order of joints
            cur = stack.pop()
            if cur not in needed:
                continue
            order.append(cur)
            stack.extend(reversed(children.get(cur, [])))
        fidx = {n: i for i, n in enumerate(order)}
        F = len(order)
        parent = np.full(F, -1, dtype=np.int32)
        jtype = np.zeros(F, dtype=np.int32)
        qidx = np.full(F, -1, dtype=np.int32)
        oxyz = np.zeros((F, 3))
        orpy = np.zeros((F, 3))
        axis = np.tile(np.array([1.0, 0.0, 0.0]), (F, 1))
        for i, name in enumerate(order):
            if name == root:
                continue
            j = urdf.parent_joint[name]
            parent[i] = fidx[j.parent]
            jtype[i] = _JTYPE[j.type]
            if j.type != "fixed":
                qidx[i] = actuated.index(j.name)
            oxyz[i] = j.xyz
            orpy[i] = j.rpy
            axis[i] = j.axis

        desc = cls(name=urdf.name, frame_names=order, parent=parent, joint_type=jtype, q_index=qidx,
                   origin_xyz=oxyz, origin_rpy=orpy, axis=axis, actuated_joint_names=actuated,
                   lower=lower, upper=upper, opt_index=opt_index, param_index=param_index, velocity=velocity, effort=effort)
        desc.frame_mass, desc.frame_com, desc.frame_inertia = lump_inertials(urdf, order)
        desc.link_names = [l.name for l in links]
        desc.link_frame = np.array([fidx[l.name] for l in links], dtype=np.int32)
        desc.visual_xyz = np.array([l.visual_xyz for l in links], dtype=np.float64).reshape(-1, 3)
        desc.visual_rpy = np.array([l.visual_rpy for l in links], dtype=np.float64).reshape(-1, 3)
        if model_dir is not None and links:
            pts, nrm, pl = [], [], []
            for li, l in enumerate(links):
                v, f = load_mesh(os.path.join(model_dir, l.visual_mesh))
                v = v * np.asarray(l.visual_scale, dtype=np.float64)[None, :]
                p, nn = sample_surface(v, f, points_per_link, seed=seed + li)
                pts.append(p)
                nrm.append(nn)
                pl.append(np.full(points_per_link, li, dtype=np.int32))
            desc.points = np.concatenate(pts)
            desc.normals = np.concatenate(nrm)
            desc.point_link = np.concatenate(pl)
        return desc

    # ------------------------------------------------------------------ fixtures
    def save(self, prefix: str) -> None:
        meta = dict(name=self.name, frame_names=self.frame_names,
                    actuated_joint_names=self.actuated_joint_names, link_names=self.link_names)
        if self.velocity is not None:  # JSON null = no limit
            meta["velocity_limits"] = [float(v) if np.isfinite(v) else None for v in self.velocity]
        with open(prefix + ".json", "w") as fh:
            json.dump(meta, fh, indent=1)
        extra = {}
        if self.effort is not None:
            extra["effort"] = self.effort
        if self.has_inertials:
            extra.update(frame_mass=self.frame_mass, frame_com=self.frame_com, frame_inertia=self.frame_inertia)
        np.savez_compressed(
            prefix + ".npz", **extra, parent=self.parent, joint_type=self.joint_type, q_index=self.q_index,
            origin_xyz=self.origin_xyz, origin_rpy=self.origin_rpy, axis=self.axis, lower=self.lower,
            upper=self.upper, opt_index=self.opt_index, param_index=self.param_index,
            link_frame=self.link_frame, visual_xyz=self.visual_xyz, visual_rpy=self.visual_rpy,
            points=self.points, normals=self.normals.astype(np.float32), point_link=self.point_link)

    @classmethod
    def load(cls, prefix: str) -> "RobotDesc":
        with open(prefix + ".json") as fh:
            meta = json.load(fh)
        z = np.load(prefix + ".npz")
        vel = meta.get("velocity_limits")  # absent in descriptions written before velocity limits were recorded
        if vel is not None:
            vel = np.array([np.inf if v is None else v for v in vel], dtype=np.float64)
        return cls(name=meta["name"], frame_names=meta["frame_names"], parent=z["parent"],
                   joint_type=z["joint_type"], q_index=z["q_index"], origin_xyz=z["origin_xyz"],
                   origin_rpy=z["origin_rpy"], axis=z["axis"],
                   actuated_joint_names=meta["actuated_joint_names"], lower=z["lower"], upper=z["upper"],
                   opt_index=z["opt_index"], param_index=z["param_index"], link_names=meta["link_names"],
                   link_frame=z["link_frame"], visual_xyz=z["visual_xyz"], visual_rpy=z["visual_rpy"],
                   points=z["points"], normals=z["normals"].astype(np.float64), point_link=z["point_link"], velocity=vel,
                   **{k: z[k] for k in ("effort", "frame_mass", "frame_com", "frame_inertia") if k in z.files})


def with_planar_base(desc: RobotDesc, xy_limit: float = 1.0, name: Optional[str] = None) -> RobotDesc:
    """The same robot on a planar mobile base: three actuated joints (prismatic x, prismatic y, revolute about z) between a
    fixed world frame and the old root, optimised together with the arm -- the mobile manipulator of
    examples/pybullet_gto_planning_mobile.py with the base pose as part of the trajectory (BASELINE configs[4]: Fetch
    arm 7 + base 3 = 10 optimised joints).  Joint order: the base joints first, then the robot's own."""
    F0 = desc.n_frames
    names = ["odom", "base_x", "base_y", "base_theta"] + list(desc.frame_names)
    parent = np.concatenate([[-1, 0, 1, 2], np.where(desc.parent < 0, 3, desc.parent + 4)]).astype(np.int32)
    jtype = np.concatenate([[JOINT_FIXED, JOINT_PRISMATIC, JOINT_PRISMATIC, JOINT_REVOLUTE], desc.joint_type]).astype(np.int32)
    qidx = np.concatenate([[-1, 0, 1, 2], np.where(desc.q_index < 0, -1, desc.q_index + 3)]).astype(np.int32)
    z3 = np.zeros((4, 3))
    axis = np.concatenate([[[1.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]], desc.axis])
    out = RobotDesc(
        name=name or desc.name + "_mobile", frame_names=names, parent=parent, joint_type=jtype, q_index=qidx,
        origin_xyz=np.concatenate([z3, desc.origin_xyz]), origin_rpy=np.concatenate([z3, desc.origin_rpy]), axis=axis,
        actuated_joint_names=["base_x", "base_y", "base_theta"] + list(desc.actuated_joint_names),
        lower=np.concatenate([[-xy_limit, -xy_limit, -np.pi], desc.lower]), upper=np.concatenate([[xy_limit, xy_limit, np.pi], desc.upper]),
        opt_index=np.concatenate([[0, 1, 2], desc.opt_index + 3]).astype(np.int32), param_index=(desc.param_index + 3).astype(np.int32),
        link_names=list(desc.link_names), link_frame=(desc.link_frame + 4).astype(np.int32), visual_xyz=desc.visual_xyz.copy(),
        visual_rpy=desc.visual_rpy.copy(), points=desc.points.copy(), normals=desc.normals.copy(), point_link=desc.point_link.copy(),
        velocity=None if desc.velocity is None else np.concatenate([[np.inf, np.inf, np.inf], desc.velocity]),
        effort=None if desc.effort is None else np.concatenate([[np.inf, np.inf, np.inf], desc.effort]))
    if desc.has_inertials:  # the base frames are massless
        out.set_link_inertials(np.concatenate([np.zeros(4), desc.frame_mass]), np.concatenate([np.zeros((4, 3)), desc.frame_com]),
                               np.concatenate([np.zeros((4, 6)), desc.frame_inertia]))
    assert out.n_frames == F0 + 4
    return out


_DATA_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def load_builtin(name: str) -> RobotDesc:
    """Distilled fixtures shipped with the package (tools/distill_robot.py): 'panda', 'fetch',
    'panda_5k' (12 x 417 points, the benchmark's ~5k-point robot)."""
    if name.endswith("_mobile"):  # 'fetch_mobile': the Fetch arm on a planar base, 10 optimised joints
        return with_planar_base(load_builtin(name[: -len("_mobile")]), name=name)
    prefix = os.path.join(_DATA_DIR, name)
    if not os.path.exists(prefix + ".npz"):
        raise FileNotFoundError(f"no built-in robot description '{name}' under {_DATA_DIR}")
    return RobotDesc.load(prefix)
