"""Write a robot URDF's inertial facts as a small JSON fixture (tests/golden/<robot>_inertials.json).

    python tools/inertials_fixture.py path/to/robot.urdf tests/golden/robot_inertials.json

Data only, read with grasptrajopt_amd.urdf: per link its mass, inertial origin (xyz, rpy) and the six inertia entries, and
the parent link with the joint origin that places it there (what lumping a pruned link into a kept frame needs,
robot_desc.lump_inertials); per joint its effort limit.  Links without mass keep their place in the tree and nothing else.
No test runs this script; tests/dynamics_ref.py reads what it wrote.
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from grasptrajopt_amd.urdf import Urdf  # noqa: E402


def fixture(urdf: Urdf) -> dict:
    links = {}
    for l in urdf.links:
        e = {}
        j = urdf.parent_joint.get(l.name)
        if j is not None:
            e.update(parent=j.parent, joint_xyz=j.xyz, joint_rpy=j.rpy)
        if l.mass > 0:
            e.update(mass=l.mass, xyz=l.inertial_xyz, rpy=l.inertial_rpy, inertia=l.inertia)
        links[l.name] = e
    joints = {j.name: {"effort": j.effort} for j in urdf.joints if j.type != "fixed"}
    return {"robot": urdf.name, "inertia_order": ["ixx", "ixy", "ixz", "iyy", "iyz", "izz"], "links": links, "joints": joints}


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with open(sys.argv[2], "w") as fh:
        json.dump(fixture(Urdf.from_file(sys.argv[1])), fh, indent=1)
