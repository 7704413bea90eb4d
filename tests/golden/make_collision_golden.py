#!/usr/bin/env python3
"""Generate tests/golden/collision_checks.npz: the reference's grasp collision filter
(examples/pybullet_gto_planning.py:203-221) and plan collision statistic (examples/pybullet_evaluate_plans.py:219-233)
on synthetic inputs, with the reference's own DepthPointCloud (mesh_to_sdf/depth_point_cloud.py: sklearn KD-tree,
get_sdf, is_outside) and the reference's forward kinematics (optas/models.py) executing at generation time through the
stand-ins of _reference_stubs.py.  Build-container only; arrays only are stored.  Re-run:
    python tests/golden/make_collision_golden.py

The scene: a camera 0.9 m behind the Panda's base looking along +x at a wall (x = 0.55) with a box in front of it
(x = 0.35 .. 0.55); everything behind the seen surfaces is "inside".  Plans run from the default pose straight to random
configurations, so some reach into the box or the wall and some do not; the grasp poses are spread over the front of
the box, so some grasps put the gripper into it.  The generator asserts what tests/test_observation_cpu.py asserts of the
fixture (both outcomes present on both checks, grazing and deep waypoints, no query on a cloud point).
"""
import os
import sys

import numpy as np
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import _reference_stubs as stubs  # noqa: E402

REF = stubs.REF


def scene():
    H, W = 120, 160
    K = np.array([[150.0, 0, 80.0], [0, 150.0, 60.0], [0, 0, 1.0]])
    cam = np.eye(4)
    cam[:3, :3] = np.array([[0, 0, 1.0], [-1.0, 0, 0], [0, -1.0, 0]])  # camera z along world x, camera x along -y, camera y along -z
    cam[:3, 3] = [-0.9, 0.0, 0.5]
    depth = np.full((H, W), 1.45, dtype=np.float32)  # the wall at x = 0.55
    depth[42:78, 56:104] = 1.25                     # the box: its front at x = 0.35
    depth[110:, 0:20] = 0.0                          # invalid pixels (a corner the robot does not reach)
    depth[:, 150:] = 2.0                             # beyond the threshold
    mask = np.zeros((H, W), dtype=np.uint8)
    mask[50:60, 70:80] = 1                           # a target on the box, dropped from the cloud
    return depth, K, cam, mask


def main():
    ref = stubs.install()
    from grasptrajopt_amd.robot_desc import load_builtin
    rng = np.random.default_rng(20241017)
    depth, K, cam, mask = scene()
    dpc = ref.dpc.DepthPointCloud(depth, K, cam, target_mask=mask, threshold=1.5)

    cfg = yaml.safe_load(open(f"{REF}/data/configs/panda.yaml"))["robot_cfg"]
    m = ref.models.RobotModel(urdf_filename=f"{REF}/{cfg['urdf_robot_path']}", time_derivs=[0, 1], param_joints=cfg["param_joints"])
    desc = load_builtin("panda")  # the 1200 surface points the GPU handle carries, in the links' visual-mesh frames
    urdf = m.get_urdf()
    vis_origin = {}
    for ln in desc.link_names:
        xyz, rpy = m.get_link_visual_origin(urdf.link_map[ln])
        vis_origin[ln] = np.asarray(ref.spatialmath.rt2tr(ref.spatialmath.rpy2r(rpy), xyz))
    link_points = [desc.points[desc.point_link == i] for i in range(desc.n_links)]

    def visual_tf(ln, q):  # gto/gto_models.py:92-100
        return np.asarray(m.get_global_link_transform(ln, q)) @ vis_origin[ln]

    def compute_fk_surface_points(q, names=None, tf_base=None):  # gto/gto_models.py:104-121, points only
        points_base_all = np.zeros((3, 0))
        for i, ln in enumerate(desc.link_names):
            if names is not None and ln not in names:
                continue
            tf = visual_tf(ln, q)
            if tf_base is not None:
                tf = tf_base @ tf
            points_base = tf[:3, :3] @ np.transpose(link_points[i]) + tf[:3, 3].reshape((3, 1))
            points_base_all = np.concatenate((points_base_all, points_base), axis=1)
        return points_base_all.T

    # ---- plans: default pose -> random configuration, straight in joint space
    lo = np.asarray(m.lower_actuated_joint_limits).ravel()
    hi = np.asarray(m.upper_actuated_joint_limits).ravel()
    qc = np.array(cfg["default_pose"], dtype=np.float64)
    B, T = 16, 50
    base_position = np.array([0.05, -0.03, 0.02])
    plans = np.zeros((B, m.ndof, T))
    for b in range(B):
        qg = qc.copy()
        qg[:7] = rng.uniform(np.maximum(lo[:7], qc[:7] - 1.2), np.minimum(hi[:7], qc[:7] + 1.2))
        plans[b] = qc[:, None] + (qg - qc)[:, None] * np.linspace(0.0, 1.0, T)[None, :]
    plan_counts = np.zeros((B, T), dtype=np.int32)
    plan_in_collision = np.zeros(B, dtype=bool)
    plan_min_abs_sdf = np.inf
    for b in range(B):
        plan = plans[b]
        in_collision = False
        for i in range(plan.shape[1]):  # examples/pybullet_evaluate_plans.py:222-233 (is_mobile False)
            q = plan[:, i]
            points_base = compute_fk_surface_points(q)
            points_world = points_base + base_position.reshape((1, 3))
            sdf = dpc.get_sdf(points_world)
            plan_counts[b, i] = np.sum(sdf < 0)
            plan_min_abs_sdf = min(plan_min_abs_sdf, float(np.abs(sdf).min()))
            if np.sum(sdf < 0) > 5:
                in_collision = True
        plan_in_collision[b] = in_collision

    # ---- grasps: the open hand (hand + fingers at the default pose) in the hand's frame, placed in front of / into the box
    hand_names = ("panda_hand", "panda_leftfinger", "panda_rightfinger")
    T_hand = np.asarray(m.get_global_link_transform("panda_hand", qc))
    gripper_points = compute_fk_surface_points(qc, hand_names, tf_base=np.linalg.inv(T_hand))
    n = 24
    poses = np.zeros((n, 4, 4))
    for i in range(n):
        c, s = np.cos(rng.uniform(-0.6, 0.6)), np.sin(rng.uniform(-0.6, 0.6))
        R = np.array([[0, 0, 1.0], [0, 1.0, 0], [-1.0, 0, 0]]) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])  # the hand's z towards the box
        poses[i, :3, :3] = R
        poses[i, :3, 3] = [rng.uniform(0.15, 0.33), rng.uniform(-0.15, 0.15), rng.uniform(0.35, 0.65)]
        poses[i, 3, 3] = 1.0
    grasp_counts = np.zeros(n, dtype=np.int32)
    grasp_in_collision = np.zeros(n, dtype=np.int32)
    grasp_min_abs_sdf = np.inf
    for i in range(n):  # examples/pybullet_gto_planning.py:207-219
        RT_off = poses[i]
        gp = RT_off[:3, :3] @ np.transpose(gripper_points) + RT_off[:3, 3].reshape((3, 1))
        sdf = dpc.get_sdf(gp.T)
        grasp_counts[i] = np.sum(sdf < 0)
        grasp_min_abs_sdf = min(grasp_min_abs_sdf, float(np.abs(sdf).min()))
        ratio = np.sum(sdf < 0) / len(sdf)
        if ratio > 0.01:
            grasp_in_collision[i] = 1

    print("plans colliding", int(plan_in_collision.sum()), "of", B, "| waypoint counts in 1..5:", int(((plan_counts >= 1) & (plan_counts <= 5)).sum()),
          "above 5:", int((plan_counts > 5).sum()), "| grasps rejected", int(grasp_in_collision.sum()), "of", n, "| min |sdf|", plan_min_abs_sdf,
          grasp_min_abs_sdf)
    assert B // 4 <= plan_in_collision.sum() <= B - B // 4
    assert ((plan_counts >= 1) & (plan_counts <= 5)).any() and (plan_counts > 5).any()
    assert 0 < grasp_in_collision.sum() < n
    assert plan_min_abs_sdf > 0 and grasp_min_abs_sdf > 0
    out = os.path.join(HERE, "collision_checks.npz")
    np.savez_compressed(out, depth=depth, K=K, cam=cam, mask=mask, threshold=np.float64(1.5), robot=np.array("panda"),
                        plans=plans, base_position=base_position, plan_counts=plan_counts, plan_in_collision=plan_in_collision,
                        plan_min_abs_sdf=np.float64(plan_min_abs_sdf), gripper_points=gripper_points, poses=poses,
                        grasp_counts=grasp_counts, grasp_in_collision=grasp_in_collision, grasp_min_abs_sdf=np.float64(grasp_min_abs_sdf))
    print(os.path.basename(out), os.path.getsize(out))


if __name__ == "__main__":
    main()
