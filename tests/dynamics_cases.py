"""The robots of the dynamics tests, CPU and GPU: (description with inertials, end-effector frame, gripper frame, gripper
points) by name.  Panda and Fetch carry the inertials of tests/golden/*_inertials.json; the others get seeded random bodies
(tests/dynamics_ref.py, one seed per robot): two trees built with tests/small_robots.py's generator, and the edge robots of
EDGE_SEEDS -- five of small_robots' kinds (one frame with an actuated root that is also the end effector, the smallest chain,
no revolute joint, an end effector above the joints, ten frames) and the chain and the bushy tree of helpers.limit_robot at
the header's capacity of 32 frames."""
import json
import os

import dynamics_ref as dr
import small_robots as sr
from grasptrajopt_amd.robot_desc import load_builtin
from helpers import limit_robot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> seed of its bodies.  Frames / what the robot is there for:
#   root_joint       1   the root is actuated (its parent's acceleration is the base's) and is frame_ee: the payload sits on it
#   chain_1          2   the smallest chain
#   prismatic_only   3   no revolute joint
#   ee_above_joints  4   frame_ee is the fixed root: the payload sits on a frame with three actuated frames below it
#   chain_9_short   10
#   limit_chain     32   depth 31, 31 degrees of freedom
#   limit_bushy     32   branches, fixed frames among them
EDGE_SEEDS = {"root_joint": 103, "chain_1": 104, "prismatic_only": 105, "ee_above_joints": 106, "chain_9_short": 107,
              "limit_chain": 108, "limit_bushy": 109}
NAMES = ("panda", "fetch", "branched", "prismatic_chain") + tuple(EDGE_SEEDS)
# (robot, payload kind of payloads()) where no joint can feel the payload, and why: the torques are the unloaded robot's
PAYLOAD_NOT_FELT = {("root_joint", "mass"): "a point mass at the origin of the revolute root lies on its axis",
                    ("chain_1", "mass"): "a point mass at the origin of the only (revolute) joint's frame lies on its axis",
                    ("ee_above_joints", "mass"): "the fixed root carries it: no joint lies between it and the base",
                    ("ee_above_joints", "full"): "the fixed root carries it: no joint lies between it and the base"}


def robot(name):
    """(desc, link_ee, link_gripper, n_gripper_points)"""
    if name in ("panda", "fetch"):
        with open(os.path.join(ROOT, "grasptrajopt_amd", "data", f"{name}_cfg.json")) as fh:
            cfg = json.load(fh)
        return dr.with_fixture_inertials(load_builtin(name), name), cfg["link_ee"], cfg["link_gripper"], None
    if name == "branched":
        # f0 fixed root; two arms split at f1, one of them splits again at f4; a fixed frame (f6) inside a branch and a
        # prismatic joint (f5) below a revolute one; the end effector (f7) is a leaf, not the last frame
        parent = [-1, 0, 1, 2, 1, 4, 5, 6, 4, 8]
        jt = [0, 1, 1, 1, 1, 2, 0, 1, 1, 1]
        d = sr._tree("branched", 11, parent, jt, list(range(10)), [3] * 10)
        return dr.random_inertials(d, 101), "f7", "f7", 3
    if name == "prismatic_chain":  # chain_7: joints 2 and 5 of 7 prismatic
        r = sr.Robot("chain_7")
        return dr.random_inertials(r.desc, 102), r.ee, r.gripper, r.n_gripper_points
    if name in ("limit_chain", "limit_bushy"):
        d, ee = limit_robot(name.split("_")[1], n_opt=16, seed=0)
        return dr.random_inertials(d, EDGE_SEEDS[name]), ee, ee, None
    if name in EDGE_SEEDS:
        r = sr.Robot(name)
        return dr.random_inertials(r.desc, EDGE_SEEDS[name]), r.ee, r.gripper, r.n_gripper_points
    raise KeyError(name)


def payloads(n, seed):
    """The three payload cases over n rows: absent, mass only, mass + com + inertia (one of the masses 0)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    mass = rng.uniform(0.2, 2.5, n)
    if n > 2:
        mass[2] = 0.0
    com = rng.uniform(-0.1, 0.1, (n, 3))
    A = rng.uniform(-0.08, 0.08, (n, 3, 3))
    I = A @ A.transpose(0, 2, 1) + 1e-4 * np.eye(3)
    six = np.stack([I[:, 0, 0], I[:, 0, 1], I[:, 0, 2], I[:, 1, 1], I[:, 1, 2], I[:, 2, 2]], axis=1)
    return {"none": None, "mass": (mass, None, None), "full": (mass, com, six)}
