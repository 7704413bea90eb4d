"""GPU: the sampled-mesh kernels (grasptrajopt_amd/csrc/gto_cloud.h, the cloud half of gto_observe.h) against the numpy FP64
restatement (tests/cloud_sdf_ref.py) and the FP64 oracle's kinematics (oracle/gto_oracle.c) on the clouds of
tests/cloud_cases.py, where the list, the tree, the skip test and the chunk loop change their path.

  a  gto_cloud_sdf_cost (SurfacePointCloud._run) on every case and every k of the case, by the tree and by the exhaustive
     search (GTO_CLOUD_BRUTE=1); Observation.sdf built and asked either way; the case's queries through check_posed at the
     identity pose (the packet walk without `order`); lattice3d's tie queries one per launch (the `<=` of the skip test)
  b  queries with NaN and infinite coordinates: what include/gto_solver.h states, the two searches bit for bit, the finite
     queries beside them unchanged
  c  gto_scene_from_clouds on a flat cloud, a ragged tree and duplicated samples, n_obstacle = k, n_all - 1, n_all
  d  check_posed on a cloud observation with 1 to 257 gripper points, and with 2^24 + 4096 queries (a second launch chain)
  e  gto_check_plans on a cloud observation: four robots, horizons with every T % 4, a shared base, per-plan bases, a NaN base,
     every GTO_CHECK_TG, the device variant on a side stream, and one plan more than a launch chain takes

Every comparison is exact; floats are compared as their bits.  In (e) the kernel's points are held to the oracle's to 1e-12
only (tests/test_gpu_limits.py), so the instances have no point within 1e-9 of a decision (cloud_cases.undecided;
tests/test_cloud_cases_cpu.py asserts it) and the counts are equal all the same.
Run the file under a time limit (timeout -k 10 600 pytest ...) and stop at the first fault."""
import time
from contextlib import nullcontext

import numpy as np
import pytest

import cloud_cases as cc
import depth_cases as dc
from helpers import exhaustive

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} differ, first at {bad[:5]}: got {got.reshape(-1)[bad[:5]]}, want {want.reshape(-1)[bad[:5]]}"


def assert_run_equals(got, e, what):
    """(sdf, inside, cost, nearest) of SurfacePointCloud._run against an expected dict."""
    assert_same_bits(got[0], e["sdf"], f"{what}: sdf")
    np.testing.assert_array_equal(got[1], e["inside"], err_msg=f"{what}: inside")
    assert_same_bits(got[2], e["cost"], f"{what}: cost")
    np.testing.assert_array_equal(got[3], e["nearest"], err_msg=f"{what}: nearest")


def searches():
    return (("tree", nullcontext), ("exhaustive", exhaustive))


# ---------------------------------------------------------------------------------------------- a. edge clouds
@pytest.mark.parametrize("name", list(cc.STATED_LEAVES))
def test_edge_clouds_equal_the_restatement(capi, name):
    import grasptrajopt_amd as g
    from grasptrajopt_amd.observation import Observation
    c = cc.cases()[name]
    cloud = g.SurfacePointCloud(c.points, c.normals)
    for k in c.ks:
        e = cc.expected(name, k)
        for search, ctx in searches():
            with ctx():
                assert_run_equals(cloud._run(c.query, k, c.epsilon, c.w_inside), e, f"k = {k}, {search}")
        for built, bctx in searches():
            with bctx():
                obs = Observation.from_cloud(c.points, c.normals, k)
            for asked, actx in searches():
                with actx():
                    sdf, inside = obs.sdf(c.query)
                    count = obs.check_posed(c.query, np.eye(4)[None])  # x = 1 x + 0 z + 0 y + 0: the queries, in the caller's order
                what = f"k = {k}, observation built by {built}, asked by {asked}"
                assert_same_bits(sdf, e["sdf"], what)
                np.testing.assert_array_equal(inside, e["inside"], err_msg=what)
                np.testing.assert_array_equal(count, [e["inside"].sum()], err_msg=what)
            obs.close()


def test_lattice3d_queries_asked_alone_need_the_box_at_the_kth_distance(capi):
    """One query per launch: no other lane of the packet opens a box for it.  The witnesses are the queries on which a walk
    that skips a box AT the k-th distance loses a tying sample of lower index (cloud_cases.lattice_witnesses)."""
    import grasptrajopt_amd as g
    c = cc.cases()["lattice3d"]
    cloud = g.SurfacePointCloud(c.points, c.normals)
    for k in cc.KS:
        e = cc.expected("lattice3d", k)
        for row in cc.lattice_witnesses()[k][:8]:
            got = cloud._run(c.query[row:row + 1], k, c.epsilon, c.w_inside)
            assert_run_equals(got, {key: v[row:row + 1] for key, v in e.items()}, f"k = {k}, query {row} alone")


# ---------------------------------------------------------------------------------------------- b. non-finite queries
@pytest.mark.parametrize("name, k", [("leaf_shapes_257", 1), ("leaf_shapes_257", 11), ("leaf_shapes_257", 13), ("lattice3d", 12),
                                     ("n_equals_k_13", 13), ("scattered", 11)])
def test_nonfinite_queries_are_answered_as_the_header_states(capi, name, k):
    import grasptrajopt_amd as g
    from grasptrajopt_amd.observation import Observation
    c = cc.cases()[name]
    q, bad_at, finite_at, kinds = cc.nonfinite_queries(c)
    cloud = g.SurfacePointCloud(c.points, c.normals)
    runs = {}
    for search, ctx in searches():
        with ctx():
            runs[search] = cloud._run(q, k, c.epsilon, c.w_inside)
            clean = cloud._run(q[finite_at], k, c.epsilon, c.w_inside)
        for a, b, what in zip(runs[search], clean, ("sdf", "inside", "cost", "nearest")):  # the finite queries are unchanged
            assert_same_bits(a[finite_at], b, f"{search}: {what} of the finite queries")
        assert_run_equals(clean, {key: v[:len(finite_at)] for key, v in cc.expected(name, k).items()}, search)
    for a, b, what in zip(runs["tree"], runs["exhaustive"], ("sdf", "inside", "cost", "nearest")):
        assert_same_bits(a, b, f"tree against exhaustive: {what}")
    sdf, inside, cost, nearest = runs["tree"]
    for row, kind in zip(bad_at, kinds):
        if kind == "nan":
            assert bits(sdf[row:row + 1])[0] == 0x7f800000 and not inside[row] and bits(cost[row:row + 1])[0] == 0 and nearest[row] == -1, (row, q[row])
        else:
            want_in = cc.lowest_indices_vote(c, q[row], k)
            assert np.isinf(sdf[row]) and (sdf[row] < 0) == want_in and inside[row] == want_in and nearest[row] == 0, (row, q[row])
            assert cost[row] == (np.inf if want_in else 0.0), (row, q[row])
    for built, bctx in searches():
        with bctx():
            obs = Observation.from_cloud(c.points, c.normals, k)
        for asked, actx in searches():
            with actx():
                o_sdf, o_in = obs.sdf(q)
            assert_same_bits(o_sdf, sdf, f"observation built by {built}, asked by {asked}: sdf")
            np.testing.assert_array_equal(o_in, inside)
        obs.close()


# ---------------------------------------------------------------------------------------------- c. scene fields
@pytest.fixture(scope="module")
def panda_handle(capi):
    from helpers import cfg_of
    from grasptrajopt_amd.robot_desc import load_builtin
    cfg = cfg_of("panda")
    h = capi.SolverHandle(load_builtin("panda"), cfg["link_ee"], cfg["link_gripper"], device=0)
    yield h
    h.close()


@pytest.mark.parametrize("sc", cc.scene_cases(), ids=lambda s: s.name)
def test_scene_fields_equal_the_restatement_at_the_voxel_centres(panda_handle, sc):
    c, h = sc.case, panda_handle
    want_shape, want_origin, q = cc.planner_grid(c.points, sc.grid_res, sc.margin)
    want_all, want_obs = cc.scene_field(sc, len(c.points))[0], cc.scene_field(sc, sc.n_obstacle)[0]
    for search, ctx in searches():
        with ctx():
            shape, origin, bounds = h.scene_from_clouds(5, c.points, c.normals, sc.n_obstacle, sc.k, sc.grid_res, sc.margin, sc.epsilon, sc.w_inside)
        assert tuple(shape) == tuple(want_shape) and len(q) <= cc.MAX_VOXELS
        np.testing.assert_array_equal(origin, want_origin)
        np.testing.assert_array_equal(bounds, np.stack((c.points.min(0), c.points.max(0)), axis=1))
        c_all, c_obs = h.scene_fields(5)
        assert_same_bits(c_all, want_all, f"c_all ({search})")
        assert_same_bits(c_obs, want_obs, f"c_obs ({search})")
    h.drop_scene(5)


# ---------------------------------------------------------------------------------------------- d. check_posed
@pytest.mark.parametrize("k", cc.POSED_KS)
@pytest.mark.parametrize("name", cc.POSED_CASES)
def test_check_posed_on_a_cloud_observation_equals_the_restatement(capi, name, k):
    from grasptrajopt_amd.observation import Observation
    c = cc.cases()[name]
    for built, bctx in searches():
        with bctx():
            obs = Observation.from_cloud(c.points, c.normals, k)
        for asked, actx in searches():
            for n_points in dc.POSED_POINTS:
                pts, RT, want = cc.posed_counts(name, n_points, k)
                with actx():
                    got = obs.check_posed(pts, RT)
                np.testing.assert_array_equal(got, want, err_msg=f"{n_points} points, built by {built}, asked by {asked}")
        obs.close()


def test_check_posed_takes_a_second_launch_chain(capi):
    """4096 gripper points at 4097 poses are 2^24 + 4096 queries: chunk_items(4097, 4096) = min(4097, kCheckChunkQueries / 4096)
    = 4096 poses go into the first launch chain (kCheckChunkQueries = 2^24, gto_api.hip) and pose 4096 alone into a second."""
    from grasptrajopt_amd.observation import Observation
    s = cc.CHUNK_POSED
    assert cc.CHUNK_QUERIES == 1 << 24 and cc.CHUNK_QUERIES // s.P == s.n - 1
    points, normals, pts, poses, want = cc.chunk_posed_instance()
    obs = Observation.from_cloud(points, normals, s.k)
    t0 = time.perf_counter()
    got = obs.check_posed(pts, poses)
    print(f"check_posed, {s.P} points x {s.n} poses: {1e3 * (time.perf_counter() - t0):.1f} ms")
    np.testing.assert_array_equal(got, want)
    obs.close()


# ---------------------------------------------------------------------------------------------- e. check_plans
def plan_setup(capi, oracle_mod, name, T):
    desc, ee, gr, ngp = dc.plan_robot(name)
    opts = oracle_mod.reference_opts(T=T, standoff_offset=-max(2, T // 5))
    h = capi.SolverHandle(desc, ee, gr, opts, device=0, n_gripper_points=ngp)
    o = oracle_mod.Oracle(desc, ee, gr, opts, n_gripper_points=ngp)
    world_points = lambda q, base: o.eval_points(0, q, base, want_field=False)[0]
    inst, want = cc.plan_case(name, T, desc, world_points)
    return desc, h, inst, want


@pytest.mark.parametrize("T", dc.PLAN_HORIZONS)
@pytest.mark.parametrize("name", dc.PLAN_ROBOTS)
def test_check_plans_on_a_cloud_observation_equals_oracle(capi, oracle_mod, monkeypatch, name, T):
    import torch
    from grasptrajopt_amd.observation import Observation
    desc, h, inst, want = plan_setup(capi, oracle_mod, name, T)
    obs = Observation.from_cloud(inst.points, inst.normals, cc.PLAN_K)
    poisoned = inst.plans.copy()
    poisoned[inst.nan_at] = np.nan
    p, _, t = inst.nan_at
    for variant, bases in (("shared", inst.base), ("per_plan", inst.bases)):
        counts, n_undecided = want[variant]
        assert n_undecided == 0 and counts[p, t] == -1
        np.testing.assert_array_equal(h.check_plans(obs, poisoned, bases), counts, err_msg=variant)
        clean = h.check_plans(obs, inst.plans, bases)  # the NaN changed nothing else
        assert clean[p, t] >= 0
        clean[p, t] = -1
        np.testing.assert_array_equal(clean, counts, err_msg=variant)
        with exhaustive():
            np.testing.assert_array_equal(h.check_plans(obs, poisoned, bases), counts, err_msg=f"{variant}, exhaustive")
    counts = want["per_plan"][0]
    # one plan's base holds a NaN: every waypoint of that plan reports -1, the other plans are unchanged
    bad_bases = inst.bases.copy()
    bad_bases[2, 1] = np.nan
    expect = counts.copy()
    expect[2] = -1
    np.testing.assert_array_equal(h.check_plans(obs, poisoned, bad_bases), expect)
    for tg in ("1", "2", "3", "4"):  # waypoints per workgroup
        monkeypatch.setenv("GTO_CHECK_TG", tg)
        np.testing.assert_array_equal(h.check_plans(obs, poisoned, inst.bases), counts, err_msg=f"GTO_CHECK_TG={tg}")
    monkeypatch.delenv("GTO_CHECK_TG")
    # the device variant on a side stream
    side = torch.cuda.Stream(device="cuda:0")
    d_plans = torch.as_tensor(poisoned, dtype=torch.float64).to("cuda:0")
    d_count = torch.full((dc.PLAN_B, T), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    h.check_plans_device(obs, dc.PLAN_B, d_plans.data_ptr(), d_count.data_ptr(), inst.base, stream=side.cuda_stream)
    side.synchronize()
    np.testing.assert_array_equal(d_count.cpu().numpy(), want["shared"][0])
    obs.close()
    h.close()


def test_check_plans_takes_a_second_launch_chain(capi, oracle_mod):
    """chain16 at T = 96: T * P = 96 * 2048 queries per plan, chunk_items(B, T * P) = min(B, kCheckChunkQueries / (T * P)) = 85
    plans per launch chain (kCheckChunkQueries = 2^24, gto_api.hip); B = 86 puts plan 85 alone into a second chain.
    Plan b is plan b % 3 of the instance."""
    from grasptrajopt_amd.observation import Observation
    name, T = cc.CHUNK_PLANS.robot, cc.CHUNK_PLANS.T
    desc, h, inst, want = plan_setup(capi, oracle_mod, name, T)
    B = cc.chunk_plans_B(desc.n_points, T)
    assert cc.CHUNK_QUERIES == 1 << 24 and (B - 1) * T * desc.n_points <= cc.CHUNK_QUERIES < B * T * desc.n_points
    assert (B, T * desc.n_points) == (86, 96 * 2048)
    obs = Observation.from_cloud(inst.points, inst.normals, cc.PLAN_K)
    poisoned = inst.plans.copy()
    poisoned[inst.nan_at] = np.nan
    pick = np.arange(B) % dc.PLAN_B
    t0 = time.perf_counter()
    got = h.check_plans(obs, poisoned[pick], inst.base)
    print(f"check_plans, {B} plans x {T} waypoints x {desc.n_points} points: {1e3 * (time.perf_counter() - t0):.1f} ms")
    np.testing.assert_array_equal(got, want["shared"][0][pick])
    obs.close()
    h.close()
