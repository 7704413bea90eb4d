"""GPU: the resident observation (gto_observation_*, gto_check_plans; grasptrajopt_amd.observation) against the paths it
replaces -- DepthPointCloud / SurfacePointCloud.get_sdf, utils.plan_in_collision, utils.grasp_collision_ratio -- and against
the reference's own counts (tests/golden/collision_checks.npz).  Every comparison is exact.  Run the file under a time limit
(timeout -k 10 900 pytest ...) and stop at the first fault."""
from contextlib import nullcontext

import numpy as np
import pytest

from conftest import golden
import cloud_sdf_ref as ref
import grasptrajopt_amd as g
from grasptrajopt_amd import _capi, surface_point_cloud as spc, synthetic as syn
from grasptrajopt_amd._capi import GTOError
from grasptrajopt_amd.observation import Observation
from grasptrajopt_amd.utils import (filter_grasps, grasp_collision_counts, grasp_collision_ratio, plan_in_collision,
                                    plans_in_collision)
from grasptrajopt_amd.synthetic import grasp_poses, random_plans, start_pose, wall_scene
from helpers import cfg_of, exhaustive

pytestmark = pytest.mark.gpu


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def robot_model(name):
    cfg = cfg_of(name)
    return g.GTORobotModel(desc=g.load_builtin(name), time_derivs=[0, 1], param_joints=cfg["param_joints"],
                           collision_link_names=cfg["collision_link_names"], device=0), cfg


def per_plan_counts(robot, cloud, plans, bases, is_mobile=False):
    """utils.plan_in_collision, plan by plan: (hit, first, counts (B, T))."""
    out = [plan_in_collision(robot, cloud, plans[b], bases[b], is_mobile=is_mobile) for b in range(len(plans))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.stack([o[2] for o in out])


@pytest.fixture(scope="module")
def depth_cloud():
    depth, K, cam, mask = wall_scene()
    return g.DepthPointCloud(depth, K, cam, target_mask=mask, threshold=1.5)


@pytest.fixture(scope="module")
def shelf_cloud():
    z = golden("surface_cloud.npz")
    pose = np.array([[-1.0, 0, 0, 0.85], [0, -1.0, 0, 0.0], [0, 0, 1.0, -0.1], [0, 0, 0, 1.0]])
    parts = [(m, T) for _, m, T in spc.urdf_visual_meshes(ref.shelf_urdf_text(z["shelf_names"], z["shelf_box_size"], z["shelf_box_xyz"]), pose)]
    crate = np.eye(4)
    crate[:3, 3] = [0.5, 0.0, 0.45]  # a solid crate in front of the shelf, within the arm's reach: boards alone are 2 cm thin
    parts.append((spc.box_mesh([0.25, 0.5, 0.3]), crate))
    pts, nrm = spc.place_meshes(parts, samples_per_m2=2.0e4, seed=3)
    return g.SurfacePointCloud(pts, nrm)


# ---------------------------------------------------------------------------------------------- 1. sdf
def test_sdf_equals_get_sdf_and_is_outside(depth_cloud):
    dpc = depth_cloud
    rng = np.random.default_rng(1)
    K, cam = dpc.intrinsic_matrix, dpc.camera_pose
    q_box = rng.uniform([-0.5, -0.8, -0.2], [1.0, 0.8, 1.2], size=(20000, 3))  # in front of and behind the surfaces, outside the view
    q_behind = rng.uniform([-2.0, -0.5, 0.0], [-0.95, 0.5, 1.0], size=(2000, 3))  # behind the camera
    # pixel coordinates in (-1, 0): truncation toward zero puts them into column / row 0
    zc = rng.uniform(0.3, 1.6, size=3000)
    u = np.where(rng.random(3000) < 0.5, rng.uniform(-1.0, 0.0, 3000), rng.uniform(0.0, dpc.width, 3000))
    v = np.where(rng.random(3000) < 0.5, rng.uniform(-1.0, 0.0, 3000), rng.uniform(0.0, dpc.height, 3000))
    pc = (np.linalg.inv(K) @ np.stack([u * zc, v * zc, zc])).T
    q_edge = pc @ cam[:3, :3].T + cam[:3, 3]
    q = np.concatenate([q_box, q_behind, q_edge])
    obs = dpc.observation()
    assert dpc.observation() is obs  # created once, cached
    sdf, inside = obs.sdf(q)
    want = dpc.get_sdf(q)
    np.testing.assert_array_equal(bits(sdf), bits(want))
    np.testing.assert_array_equal(inside, ~dpc.is_outside(q))
    assert inside.any() and (~inside).any() and inside[-3000:].any() and (~inside[-3000:]).any()
    # any batch, any position: the same bits
    sdf1, in1 = obs.sdf(q[777:778])
    assert bits(sdf1)[0] == bits(sdf)[777] and in1[0] == inside[777]
    s0, i0 = obs.sdf(np.zeros((0, 3)))
    assert s0.shape == (0,) and i0.shape == (0,)


def test_cloud_sdf_equals_get_sdf(shelf_cloud):
    rng = np.random.default_rng(2)
    lo, hi = shelf_cloud.points.min(0) - 0.3, shelf_cloud.points.max(0) + 0.3
    q = rng.uniform(lo, hi, size=(30000, 3))
    for k in (11, 1):
        obs = shelf_cloud.observation(k)
        sdf, inside = obs.sdf(q)
        want = shelf_cloud.get_sdf(q, sample_count=k)
        np.testing.assert_array_equal(bits(sdf), bits(want))
        np.testing.assert_array_equal(inside, want < 0)
        assert inside.any() and (~inside).any()


# ---------------------------------------------------------------------------------------------- 2. plans
@pytest.mark.parametrize("B", [1, 7, 64])
@pytest.mark.parametrize("name", ["panda_5k", "fetch"])
def test_check_plans_equals_plan_in_collision(name, B, depth_cloud):
    robot, cfg = robot_model(name)
    if name == "fetch":  # the Fetch's arm sits higher and further forward: the camera is moved with it
        depth, K, cam, mask = wall_scene(cam_xyz=(-0.8, 0.0, 0.9))
        dpc = g.DepthPointCloud(depth, K, cam, target_mask=mask, threshold=1.5)
    else:
        dpc = depth_cloud
    plans = random_plans(robot.desc, cfg, B, seed=10 + B)
    rng = np.random.default_rng(B)
    base = np.array([0.05, -0.03, 0.02])
    bases = rng.uniform(-0.08, 0.08, size=(B, 3))
    obs = dpc.observation()
    # one non-zero base for all plans
    hit, first, counts = plans_in_collision(robot, dpc, plans, base)
    w_hit, w_first, w_counts = per_plan_counts(robot, dpc, plans, np.tile(base, (B, 1)))
    np.testing.assert_array_equal(counts, w_counts)
    np.testing.assert_array_equal(hit, w_hit)
    np.testing.assert_array_equal(first, w_first)
    assert counts.dtype == np.int32 and counts.shape == (B, 50)
    # a base per plan
    _, _, counts_pp = plans_in_collision(robot, obs, plans, bases)
    np.testing.assert_array_equal(counts_pp, per_plan_counts(robot, dpc, plans, bases)[2])
    # is_mobile: the base is ignored
    _, _, counts_m = plans_in_collision(robot, obs, plans, base, is_mobile=True)
    np.testing.assert_array_equal(counts_m, per_plan_counts(robot, dpc, plans, np.tile(base, (B, 1)), is_mobile=True)[2])
    np.testing.assert_array_equal(counts_m, plans_in_collision(robot, obs, plans, np.zeros(3))[2])
    if B == 64:
        assert hit.any() and (~hit).any() and ((w_counts >= 1) & (w_counts <= 5)).any()
    robot.close()


def test_check_plans_equals_the_reference_counts_through_the_c_abi():
    z = golden("collision_checks.npz")
    cfg = cfg_of("panda")
    h = _capi.SolverHandle(g.load_builtin("panda"), cfg["link_ee"], cfg["link_gripper"], device=0)
    obs = Observation.from_depth(z["depth"], z["K"], z["cam"], z["mask"], float(z["threshold"]))
    counts = h.check_plans(obs, z["plans"], z["base_position"])
    np.testing.assert_array_equal(counts, z["plan_counts"])
    np.testing.assert_array_equal((counts > 5).any(axis=1), z["plan_in_collision"])
    np.testing.assert_array_equal(obs.check_posed(z["gripper_points"], z["poses"]), z["grasp_counts"])
    obs.close()
    h.close()


# ---------------------------------------------------------------------------------------------- 3. grasps
def test_check_posed_equals_grasp_collision_ratio(depth_cloud):
    robot, cfg = robot_model("panda_5k")
    qc = start_pose(robot.desc, cfg)
    RT = grasp_poses(64, 3)  # the whole robot at its default pose stands in for the gripper model
    off = syn.standoff_pose(-0.1, cfg["axis_standoff"])
    for RT_offset in (None, off):
        ratio = grasp_collision_ratio(robot, depth_cloud, RT, qc, RT_offset)
        counts, P = grasp_collision_counts(robot, depth_cloud, RT, qc, RT_offset)
        assert P == robot.desc.n_points and counts.dtype == np.int32
        np.testing.assert_array_equal(counts / P, ratio)
        np.testing.assert_array_equal((counts / P > 0.01).astype(np.int32), filter_grasps(robot, depth_cloud, RT, qc, RT_offset))
        assert (ratio > 0.01).any() and (ratio <= 0.01).any()
    # any batch, any position; an empty batch
    obs = depth_cloud.observation()
    pts, _ = robot.compute_fk_surface_points(qc)
    all_ = obs.check_posed(pts, RT)
    assert obs.check_posed(pts, RT[17:18])[0] == all_[17]
    np.testing.assert_array_equal(obs.check_posed(pts, np.concatenate([RT[40:], RT[:40]])), np.concatenate([all_[40:], all_[:40]]))
    assert obs.check_posed(pts, np.zeros((0, 4, 4))).shape == (0,)
    bad = RT.copy()
    bad[5, 1, 3] = np.nan
    got = obs.check_posed(pts, bad)
    assert got[5] == -1 and np.array_equal(np.delete(got, 5), np.delete(all_, 5))
    robot.close()


# ---------------------------------------------------------------------------------------------- 4. device variant
def test_device_variant_takes_the_solvers_output_on_its_stream(depth_cloud):
    import torch
    cfg = cfg_of("panda")
    desc = g.load_builtin("panda")
    h = _capi.SolverHandle(desc, cfg["link_ee"], cfg["link_gripper"], device=0)
    B = 8
    sc = syn.make_scene(3, n=48, res=0.0467)
    h.set_scene(0, sc.c_all, sc.c_obs, sc.shape, sc.origin, sc.res)
    RT, qg = syn.make_goals(desc, h.eval_fk, cfg["link_ee"], B, seed=5)
    qc = np.array(cfg["default_pose"])
    Q0 = np.stack([syn.make_seed(qc, qg[i], h.T, desc.param_index) for i in range(B)])
    S = syn.standoff_pose(-0.1, cfg["axis_standoff"])
    h.set_opts(max_iter=30)
    cu = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to("cuda:0")
    sid, ng = cu(np.zeros(B), torch.int32), cu(np.ones(B), torch.int32)
    keep = [cu(np.tile(qc, (B, 1))), cu(RT.reshape(B, 1, 16)), cu(np.tile(S.reshape(1, 16), (B, 1))), cu(np.zeros((B, 3))), cu(Q0)]
    Qd = torch.empty((B, desc.ndof, 50), dtype=torch.float64, device="cuda:0")
    cnt = torch.full((B, 50), -7, dtype=torch.int32, device="cuda:0")
    obs = depth_cloud.observation()
    base = np.array([0.3, 0.02, 0.0])  # pushed towards the box so that some waypoints touch it
    torch.cuda.synchronize()
    h.solve_batch_device(B, 1, sid.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), ng.data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(),
                         keep[4].data_ptr(), Qd.data_ptr(), None, None, None, None)
    h.check_plans_device(obs, B, Qd.data_ptr(), cnt.data_ptr(), base)  # same stream, nothing in between
    torch.cuda.synchronize()
    Qh, got = Qd.cpu().numpy(), cnt.cpu().numpy()
    np.testing.assert_array_equal(got, h.check_plans(obs, Qh, base))
    assert (got >= 0).all() and (got > 0).any()
    h.close()


# ---------------------------------------------------------------------------------------------- 5 - 7
def test_batch_independence_nan_and_errors(depth_cloud):
    robot, cfg = robot_model("panda_5k")
    obs = depth_cloud.observation()
    h = robot._util_handle()
    base = np.array([0.05, -0.03, 0.02])
    plans = random_plans(robot.desc, cfg, 4096, seed=99)
    big = h.check_plans(obs, plans, base)
    for pos in (0, 2048, 4095):
        np.testing.assert_array_equal(h.check_plans(obs, plans[pos:pos + 1], base)[0], big[pos])
    moved = plans[[4095, 7, 2048, 0]]
    np.testing.assert_array_equal(h.check_plans(obs, moved, base), big[[4095, 7, 2048, 0]])
    assert h.check_plans(obs, np.zeros((0, robot.desc.ndof, 50)), base).shape == (0, 50)  # B = 0: no launch
    # waypoints per workgroup (GTO_CHECK_TG, read by every call): the same counts
    import os
    for tg in ("1", "2", "3"):
        os.environ["GTO_CHECK_TG"] = tg
        try:
            np.testing.assert_array_equal(h.check_plans(obs, plans[:65], base), big[:65])
        finally:
            del os.environ["GTO_CHECK_TG"]
    # a NaN in one waypoint: -1 there, nothing else changes
    few = plans[:9].copy()
    few[4, 3, 21] = np.nan
    got = h.check_plans(obs, few, base)
    want = big[:9].copy()
    want[4, 21] = -1
    np.testing.assert_array_equal(got, want)
    hit, first, _ = plans_in_collision(robot, obs, few, base)
    np.testing.assert_array_equal(hit, (want > 5).any(axis=1))
    # errors name their cause
    with pytest.raises(GTOError, match="horizon T = 50"):
        h.check_plans(obs, plans[:2, :, :40], base)
    with pytest.raises(GTOError, match="one base per plan"):
        h.check_plans(obs, plans[:2], np.zeros((3, 3)))
    import torch
    if torch.cuda.device_count() > 1:
        other = Observation.from_depth(depth_cloud.depth, depth_cloud.intrinsic_matrix, depth_cloud.camera_pose, device=1)
        with pytest.raises(GTOError, match="another device"):
            h.check_plans(other, plans[:2], base)
        other.close()
    gone = Observation.from_depth(depth_cloud.depth, depth_cloud.intrinsic_matrix, depth_cloud.camera_pose)
    gone.close()
    with pytest.raises(GTOError, match="closed"):
        h.check_plans(gone, plans[:2], base)
    with pytest.raises(GTOError, match="closed"):
        gone.sdf(np.zeros((1, 3)))
    robot.close()


# ---------------------------------------------------------------------------------------------- 8. cloud observation
def test_cloud_observation_checks(shelf_cloud):
    robot, cfg = robot_model("panda")
    obs = shelf_cloud.observation()
    assert obs.kind == "cloud" and shelf_cloud.observation() is obs
    base = np.array([0.1, 0.01, 0.0])
    for B in (1, 7, 64):
        plans = random_plans(robot.desc, cfg, B, seed=20 + B, reach=1.5)
        bases = np.random.default_rng(B).uniform(-0.05, 0.05, size=(B, 3))
        hit, first, counts = plans_in_collision(robot, shelf_cloud, plans, base)
        w_hit, w_first, w_counts = per_plan_counts(robot, shelf_cloud, plans, np.tile(base, (B, 1)))
        np.testing.assert_array_equal(counts, w_counts)
        np.testing.assert_array_equal(hit, w_hit)
        np.testing.assert_array_equal(first, w_first)
        np.testing.assert_array_equal(plans_in_collision(robot, obs, plans, bases)[2], per_plan_counts(robot, shelf_cloud, plans, bases)[2])
        np.testing.assert_array_equal(plans_in_collision(robot, obs, plans, base, is_mobile=True)[2],
                                      per_plan_counts(robot, shelf_cloud, plans, np.tile(base, (B, 1)), is_mobile=True)[2])
    assert w_counts.max() > 5 and (w_counts == 0).any(), w_counts.max()
    # grasps
    qc = start_pose(robot.desc, cfg)
    RT = grasp_poses(64, 4, x=(-0.2, 0.5))
    ratio = grasp_collision_ratio(robot, shelf_cloud, RT, qc)
    counts, P = grasp_collision_counts(robot, shelf_cloud, RT, qc)
    np.testing.assert_array_equal(counts / P, ratio)
    np.testing.assert_array_equal((counts / P > 0.01).astype(np.int32), filter_grasps(robot, shelf_cloud, RT, qc))
    assert (ratio > 0.01).any()
    # batch independence, an empty batch, a NaN
    h = robot._util_handle()
    plans = random_plans(robot.desc, cfg, 4096, seed=98, reach=1.5)
    big = h.check_plans(obs, plans, base)
    for pos in (0, 2048, 4095):
        np.testing.assert_array_equal(h.check_plans(obs, plans[pos:pos + 1], base)[0], big[pos])
    assert h.check_plans(obs, np.zeros((0, robot.desc.ndof, 50)), base).shape == (0, 50)
    few = plans[:5].copy()
    few[2, 0, 49] = np.inf
    want = big[:5].copy()
    want[2, 49] = -1
    np.testing.assert_array_equal(h.check_plans(obs, few, base), want)
    robot.close()


# ---------------------------------------------------------------------------------------------- 9. cloud observation, both searches
@pytest.mark.parametrize("k", [1, 11])
@pytest.mark.parametrize("n", [11, 33, 65])
def test_cloud_observation_by_tree_and_by_exhaustive_search(n, k, monkeypatch):
    """One leaf that is not full, two leaves, three leaves.  Whether the observation was built with its hierarchy or under
    GTO_CLOUD_BRUTE=1 without one, and whether it is asked with the variable set or not: sdf gives the restatement's bits,
    and check_posed the restatement's counts (poses of identity rotation: the kernel's position is q + t in float64, one
    rounding, as numpy's).  257 points cross the 256-thread stride of the check."""
    monkeypatch.delenv("GTO_CLOUD_BRUTE", raising=False)
    rng = np.random.default_rng(n)
    pts, nrm = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    q = np.concatenate([rng.normal(size=(300, 3)), pts[:5], 50.0 + rng.normal(size=(10, 3))])
    want = ref.cloud_sdf(pts, nrm, q, k=k)
    poses = np.tile(np.eye(4), (8, 1, 1))
    poses[:, :3, 3] = rng.normal(size=(8, 3))
    want_counts = np.array([ref.cloud_sdf(pts, nrm, q[:257] + t, k=k)["inside"].sum() for t in poses[:, :3, 3]], dtype=np.int32)
    assert (want_counts > 0).any() and (want_counts < 257).any()
    poses[6, 2, 3] = np.nan
    want_counts[6] = -1
    for built_brute in (False, True):
        with exhaustive() if built_brute else nullcontext():
            obs = Observation.from_cloud(pts, nrm, k)
        for asked_brute in (False, True):
            with exhaustive() if asked_brute else nullcontext():
                sdf, inside = obs.sdf(q)
                counts = obs.check_posed(q[:257], poses)
            mode = f"built exhaustive={built_brute}, asked exhaustive={asked_brute}"
            np.testing.assert_array_equal(bits(sdf), bits(want["sdf"]), err_msg=mode)
            np.testing.assert_array_equal(inside, want["inside"], err_msg=mode)
            np.testing.assert_array_equal(counts, want_counts, err_msg=mode)
        obs.close()
