"""GPU: cost fields from sampled triangle meshes (gto_cloud_sdf_cost, gto_scene_from_clouds, SurfacePointCloud) against the
reference's own results (tests/golden/surface_cloud.npz, made by tests/golden/make_surface_cloud_golden.py) and the numpy
restatement (cloud_sdf_ref.py), and through the planner.  Run the file under a time limit (timeout -k 10 600 pytest ...)
and stop at the first fault."""
import numpy as np
import pytest

from conftest import golden
import cloud_sdf_ref as ref
import grasptrajopt_amd as g
from grasptrajopt_amd import surface_point_cloud as spc
from grasptrajopt_amd import synthetic as syn
from helpers import cfg_of, exhaustive

pytestmark = pytest.mark.gpu


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def shelf_parts(z, base_pose=None):
    return [(m, T) for _, m, T in spc.urdf_visual_meshes(ref.shelf_urdf_text(z["shelf_names"], z["shelf_box_size"], z["shelf_box_xyz"]),
                                                         base_pose)]


@pytest.mark.parametrize("k", [11, 1])
@pytest.mark.parametrize("name", ["table", "shelf"])
def test_cloud_sdf_cost_equals_the_reference_bit_for_bit(name, k):
    z = golden("surface_cloud.npz")
    pts, nrm = ref.unpack_cloud(z, name)
    want = z[f"{name}_sdf_k{k}"]
    mine = ref.cloud_sdf(pts, nrm, z[f"{name}_query"], k=k)
    sdf, inside, cost, nearest = g.SurfacePointCloud(pts, nrm)._run(z[f"{name}_query"], k, 0.02, 1.0)
    np.testing.assert_array_equal(bits(sdf), bits(want))
    np.testing.assert_array_equal(inside, want < 0)
    np.testing.assert_array_equal(bits(cost), bits(ref.cost_map(want, want < 0, 0.02, 1.0)))
    np.testing.assert_array_equal(nearest, mine["nearest"])
    cost3 = g.SurfacePointCloud(pts, nrm).get_sdf_cost(z[f"{name}_query"], epsilon=0.05, w_inside=3, sample_count=k)
    np.testing.assert_array_equal(bits(cost3), bits(ref.cost_map(want, want < 0, 0.05, 3.0)))
    assert (cost > 0).any() and (cost == 0).any()


def test_get_voxels_equals_the_reference():
    z = golden("surface_cloud.npz")
    for name in ("table", "shelf"):
        pts, nrm = ref.unpack_cloud(z, name)
        vox = g.SurfacePointCloud(ref.unit_cube_cloud(pts), nrm).get_voxels(16)
        np.testing.assert_array_equal(bits(vox), bits(z[f"{name}_voxels16"]))
        assert g.SurfacePointCloud(ref.unit_cube_cloud(pts), nrm).get_voxels(16, pad=True).shape == (18, 18, 18)


@pytest.mark.parametrize("k", [1, 5, 11, 16])
def test_tree_search_equals_exhaustive_search_on_ties(k):
    """Every sample stored twice, and queries exactly on samples: the k-th and (k+1)-th neighbour tie all the time, and
    (distance, index) decides.  The tree search, the exhaustive search and the restatement agree on every output."""
    z = golden("surface_cloud.npz")
    pts, nrm = ref.unpack_cloud(z, "shelf")
    pts, nrm = np.concatenate([pts, pts]), np.concatenate([nrm, -nrm])  # (the twin votes the other way: a vote that flips
    q = np.concatenate([pts[:1500], z["shelf_query"][:1500]])           # with the tie-break shows in `inside`)
    cloud = g.SurfacePointCloud(pts, nrm)
    tree = cloud._run(q, k, 0.02, 1.0)
    with exhaustive():
        brute = cloud._run(q, k, 0.02, 1.0)
    for a, b in zip(tree, brute):
        np.testing.assert_array_equal(a.view(np.uint8) if a.dtype == bool else a, b.view(np.uint8) if b.dtype == bool else b)
    mine = ref.cloud_sdf(pts, nrm, q, k=k)
    np.testing.assert_array_equal(bits(tree[0]), bits(mine["sdf"]))
    np.testing.assert_array_equal(tree[1], mine["inside"])
    np.testing.assert_array_equal(tree[3], mine["nearest"])
    assert (tree[3][:1500] == np.arange(1500)).all()  # a query on a sample: the first of the two twins is the nearest


@pytest.mark.parametrize("n", [11, 12, 33, 64, 65, 1000])
def test_small_clouds(n):
    """One leaf, a leaf that is not full, a tree of two and three leaves: tree, exhaustive search and restatement agree."""
    rng = np.random.default_rng(n)
    pts, nrm = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    q = np.concatenate([rng.normal(size=(300, 3)), pts[:5], 50.0 + rng.normal(size=(10, 3))])
    cloud = g.SurfacePointCloud(pts, nrm)
    for k in (1, 11):
        mine = ref.cloud_sdf(pts, nrm, q, k=k)
        tree = cloud._run(q, k, 0.02, 1.0)
        with exhaustive():
            brute = cloud._run(q, k, 0.02, 1.0)
        for got in (tree, brute):
            np.testing.assert_array_equal(bits(got[0]), bits(mine["sdf"]))
            np.testing.assert_array_equal(got[1], mine["inside"])
            np.testing.assert_array_equal(got[3], mine["nearest"])


def planner_grid(points, res=0.05, margin=0.4):
    """gto/gto_models.py:155-171."""
    lo, hi = points.min(0), points.max(0)
    axes = [np.arange(lo[a] - margin, hi[a] + margin, res) for a in range(3)]
    wp = np.array(np.meshgrid(*axes, indexing="ij"))
    return wp.shape[1:], np.array([lo[a] - margin for a in range(3)]), wp.reshape((3, -1)).T


def test_shelf_field_at_realistic_size():
    """The shelf at about 3 x 10^5 samples on the planner's grid (0.05 m, margin 0.4 m).

    Spacing bound.  With rho samples per m^2 drawn uniformly, a surface point has no sample within r with probability
    exp(-rho pi r^2 / 4) at worst (at a corner of a board a quarter of the disc lies on the face).  r is chosen so that the
    expected number of voxels whose nearest surface point is that unlucky is 10^-3: r^2 = 4 ln(10^3 N_voxels) / (pi rho).
    The nearest sample of a voxel at true distance d is then within sqrt(d^2 + r^2) <= d + r.

    Sign bound.  The share of voxels whose sign differs from the analytic one may be no larger than the upper end of the
    three-sigma Wilson score interval of the share the reference restatement shows on a random sample of 2048 voxels: the
    three-sigma bound of a binomial share that stays meaningful when the sample shows none."""
    z = golden("surface_cloud.npz")
    parts = shelf_parts(z)
    area = sum(spc.mesh_area(*m) for m, _ in parts)
    pts, nrm = spc.place_meshes(parts, samples_per_m2=3.0e5 / area, seed=5)
    assert 3.0e5 <= len(pts) <= 3.0e5 + 6
    np.testing.assert_allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-12)
    shape, origin, wp = planner_grid(pts)
    sdf, inside, cost, nearest = g.SurfacePointCloud(pts, nrm)._run(wp, 11, 0.02, 1.0)
    pick = np.random.default_rng(7).choice(len(wp), 2048, replace=False)
    mine = ref.cloud_sdf(pts, nrm, wp[pick], k=11, chunk=32)
    np.testing.assert_array_equal(bits(sdf[pick]), bits(mine["sdf"]))
    np.testing.assert_array_equal(nearest[pick], mine["nearest"])
    np.testing.assert_array_equal(bits(cost[pick]), bits(ref.cost_map(mine["sdf"], mine["inside"])))
    exact = ref.box_union_sdf(wp, z["shelf_box_xyz"], z["shelf_box_size"])
    rho = len(pts) / area
    spacing = np.sqrt(4.0 * np.log(1.0e3 * len(wp)) / (np.pi * rho))
    err = np.abs(np.abs(sdf.astype(np.float64)) - np.abs(exact))
    print(f"voxels {len(wp)}, samples {len(pts)}, spacing bound {spacing:.5f} m, max | |sdf| - |exact| | {err.max():.5f} m")
    assert err.max() <= spacing + 1e-6  # (+ float32 rounding of the distance)
    wrong_ref = float(((mine["sdf"] < 0) != (exact[pick] < 0)).mean())
    zs, n = 3.0, 2048.0
    upper = (wrong_ref + zs * zs / (2 * n) + zs * np.sqrt(wrong_ref * (1 - wrong_ref) / n + zs * zs / (4 * n * n))) / (1 + zs * zs / n)
    wrong = float(((sdf < 0) != (exact < 0)).mean())
    print(f"sign differs from the analytic one: restatement on the sample {wrong_ref:.3e}, three-sigma upper end {upper:.3e}, "
          f"GPU on all voxels {wrong:.3e}")
    assert wrong <= upper


def panda_handle():
    from grasptrajopt_amd import _capi
    cfg = cfg_of("panda")
    return _capi.SolverHandle(g.load_builtin("panda"), cfg["link_ee"], cfg["link_gripper"], device=0)


def test_scene_from_clouds_equals_two_stand_alone_calls():
    z = golden("surface_cloud.npz")
    pts, nrm = ref.unpack_cloud(z, "shelf")
    n_obs = int(z["shelf_counts"][:4].sum())  # the scene without its last two boards
    h = panda_handle()
    for res, margin, k in ((0.05, 0.4, 11), (0.031, 0.13, 1)):
        shape, origin, bounds = h.scene_from_clouds(3, pts, nrm, n_obs, k, res, margin, 0.03, 2.0)
        want_shape, want_origin, wp = planner_grid(pts, res, margin)
        assert tuple(shape) == tuple(want_shape)
        np.testing.assert_array_equal(origin, want_origin)
        np.testing.assert_array_equal(bounds, np.stack((pts.min(0), pts.max(0)), axis=1))
        c_all, c_obs = h.scene_fields(3)
        np.testing.assert_array_equal(bits(c_all), bits(g.SurfacePointCloud(pts, nrm).get_sdf_cost(wp, 0.03, 2.0, sample_count=k)))
        np.testing.assert_array_equal(bits(c_obs), bits(g.SurfacePointCloud(pts[:n_obs], nrm[:n_obs]).get_sdf_cost(wp, 0.03, 2.0, sample_count=k)))
        assert (c_all != c_obs).any()
        with exhaustive():
            h.scene_from_clouds(4, pts, nrm, n_obs, k, res, margin, 0.03, 2.0)
        b_all, b_obs = h.scene_fields(4)
        np.testing.assert_array_equal(bits(b_all), bits(c_all))
        np.testing.assert_array_equal(bits(b_obs), bits(c_obs))
    h.scene_from_clouds(3, pts, nrm, None, 11, 0.05, 0.4, 0.03, 2.0)
    one_all, one_obs = h.scene_fields(3)
    np.testing.assert_array_equal(bits(one_all), bits(one_obs))
    from grasptrajopt_amd._capi import GTOError
    with pytest.raises(GTOError, match="fewer samples than k"):
        h.scene_from_clouds(3, pts[:5], nrm[:5], None, 11)
    with pytest.raises(GTOError, match="n_obstacle must be <= n_all"):
        h.scene_from_clouds(3, pts, nrm, len(pts) + 1, 11)
    bad = pts.copy()
    bad[17, 1] = np.nan
    with pytest.raises(GTOError, match="non-finite"):
        h.scene_from_clouds(3, bad, nrm, None, 11)
    h.scene_from_clouds(3, pts, nrm, None, 11)  # and the next call is served
    h.close()


def test_plan_into_the_mesh_shelf_through_the_resident_scene():
    """Panda in front of the shelf (its opening towards the robot) with a box on the middle board, 64 goal grasps above the
    box: plan_goalset through the resident mesh scene (setup_clouds_field) returns what it returns for the same two fields
    uploaded as arrays, bit for bit, and the plan is collision-free by the reference's criterion (at no waypoint more than
    5 surface points of the robot inside the obstacles, examples/pybullet_evaluate_plans.py:219-233)."""
    from grasptrajopt_amd.utils import grasp_collision_ratio, plan_in_collision
    z = golden("surface_cloud.npz")
    cfg = cfg_of("panda")
    pose = np.array([[-1.0, 0, 0, 0.85], [0, -1.0, 0, 0.0], [0, 0, 1.0, -0.1], [0, 0, 0, 1.0]])  # turned by pi about z
    parts = shelf_parts(z, pose)
    pts, nrm = spc.place_meshes(parts, samples_per_m2=2.0e4, seed=3)
    shelf = g.SurfacePointCloud(pts, nrm)
    box_pose = np.eye(4)
    box_pose[:3, 3] = [0.74, 0.0, -0.1 + 0.3905 + 0.011 + 0.05]  # standing on the middle board
    tp, tn = spc.place_meshes([(spc.box_mesh([0.05, 0.05, 0.1]), box_pose)], samples_per_m2=2.0e4, seed=4)
    target = g.SurfacePointCloud(tp, tn)
    qc = np.array(cfg["default_pose"])
    out = {}
    for path in ("resident", "uploaded"):
        robot = g.GTORobotModel(desc=g.load_builtin("panda"), time_derivs=[0, 1], param_joints=cfg["param_joints"],
                                collision_link_names=cfg["collision_link_names"], device=0)
        c_all, c_obs = robot.setup_clouds_field(shelf, target)
        assert not isinstance(c_all, np.ndarray) and c_all.resident() is not None and c_obs.resident().half == 1
        if path == "uploaded":
            c_all, c_obs = np.array(c_all), np.array(c_obs)
            wp = robot.workspace_points
            both = g.SurfacePointCloud(np.concatenate([pts, tp]), np.concatenate([nrm, tn]))
            np.testing.assert_array_equal(bits(c_all), bits(both.get_sdf_cost(wp)))
            np.testing.assert_array_equal(bits(c_obs), bits(shelf.get_sdf_cost(wp)))

        def touches(q):  # the reference's pipeline only passes collision-free grasp configurations on
            xyz, _, _, _ = robot._util_handle().eval_points(0, q, [0, 0, 0], want_field=False)
            return (shelf.get_sdf(xyz.reshape(-1, 3)).reshape(len(q), -1) < 0).sum(axis=1).astype(np.float64)

        RT, q_goal = syn.make_goals(robot.desc, robot._util_handle().eval_fk, cfg["link_ee"], 64, seed=21, xlim=(0.55, 0.72),
                                    ylim=(-0.2, 0.2), zlim=(0.45, 0.6), collision_cost=touches)
        planner = g.GTOPlanner(robot, cfg["link_ee"], cfg["link_gripper"], standoff_distance=-0.1, standoff_offset=-10)
        plan, dQ, cost = planner.plan_goalset(qc, RT, c_all, c_obs, [0.0, 0.0, 0.0], q_goal.T.astype(np.float32),
                                              use_standoff=True, axis_standoff=cfg["axis_standoff"], interpolate=True)
        stats = planner.solver.stats()
        hit, first, count = plan_in_collision(robot, shelf, plan, [0.0, 0.0, 0.0])
        print(f"{path}: cost {cost}, iterations {stats['iter_count']}, {stats['return_status']}, seed {planner.seed_index}, "
              f"robot points inside the shelf per waypoint: max {count.max()}")
        ratio = grasp_collision_ratio(robot, shelf, RT, qc)
        assert ratio.shape == (64,) and ((ratio >= 0) & (ratio <= 1)).all()
        out[path] = dict(plan=plan, dQ=dQ, cost=cost, it=stats["iter_count"], status=stats["return_status"], hit=hit, count=count)
        robot.close()
    a, b = out["resident"], out["uploaded"]
    np.testing.assert_array_equal(a["plan"], b["plan"])
    np.testing.assert_array_equal(a["dQ"], b["dQ"])
    np.testing.assert_array_equal(a["cost"], b["cost"])
    assert (a["it"], a["status"]) == (b["it"], b["status"])
    assert not a["hit"], f"the plan collides: robot points inside the shelf per waypoint {a['count'].tolist()}"
