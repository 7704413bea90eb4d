"""GPU: the depth-image kernels (grasptrajopt_amd/csrc/gto_depth.h, gto_observe.h) against the FP64 oracle
(oracle/gto_oracle.c) at the image shapes of tests/depth_cases.py, where tile, wave and tree bookkeeping change their path:
a hierarchy of one leaf, strips one pixel wide, the largest hierarchy k_bvh_up builds and the image beyond it, clouds of
one point, of none and of zero extent in an axis.

  a  gto_depth_sdf_cost (DepthPointCloud) on every case, by the tree and by the exhaustive search (GTO_DEPTH_BRUTE=1)
  b  gto_scene_from_depth on the small cases: the cost-only search (k_depth_sdf_bvh, cost_only) at the voxel centres of its
     own grid, both fields, with a target mask and with a separate obstacle image; two grids whose centres lie on the
     boundary dist < epsilon to within rounding
  c  the resident observation on every case: sdf, and check_posed with 1 to 257 gripper points
  d  gto_check_plans on a depth observation: four robots, horizons with every T % 4, a shared base and one per plan

Every comparison is exact; floats are compared as their bits (-0.0 and inf count).  In (d) the kernel's points are held to
the oracle's to 1e-12 only (tests/test_gpu_limits.py), so the instances are chosen to have no point within 1e-9 of a
decision (depth_cases.undecided; tests/test_depth_cases_cpu.py asserts it) and the counts are equal all the same.
Run the file under a time limit (timeout -k 10 600 pytest ...) and stop at the first fault."""
import numpy as np
import pytest

import depth_cases as dc

pytestmark = pytest.mark.gpu

CASES = list(dc.STATED_P)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} differ, first at {bad[:5]}: got {got.reshape(-1)[bad[:5]]}, want {want.reshape(-1)[bad[:5]]}"


_ORACLE = {}


def oracle_field(oracle_mod, key, depth, K, cam, mask, threshold, query, epsilon, w_inside):
    """oracle.depth_sdf_cost, computed once per key and left unchanged."""
    if key not in _ORACLE:
        out = oracle_mod.depth_sdf_cost(depth, K, cam, mask, threshold, query, epsilon=epsilon, w_inside=w_inside)
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def oracle_of_case(oracle_mod, c):
    return oracle_field(oracle_mod, ("case", c.name), c.depth, c.K, c.cam, c.mask, c.threshold, c.query, c.epsilon, c.w_inside)


# ---------------------------------------------------------------------------------------------- a. stand-alone field
@pytest.mark.parametrize("search", ["tree", "brute"])
@pytest.mark.parametrize("name", CASES)
def test_stand_alone_field_equals_oracle(capi, oracle_mod, monkeypatch, name, search):
    import grasptrajopt_amd as g
    c = dc.cases()[name]
    pts, sdf, inside, cost = oracle_of_case(oracle_mod, c)
    monkeypatch.setenv("GTO_DEPTH_BRUTE", "1" if search == "brute" else "0")
    dpc = g.DepthPointCloud(c.depth, c.K, c.cam, target_mask=c.mask, threshold=c.threshold)
    assert_same_bits(np.asarray(dpc.points), pts, "points")
    got = dpc.get_sdf(c.query)
    assert_same_bits(got, sdf, "get_sdf")
    np.testing.assert_array_equal(dpc.is_outside(c.query), ~inside)
    assert_same_bits(dpc.get_sdf_cost(c.query, epsilon=c.epsilon, w_inside=c.w_inside), cost, "get_sdf_cost")
    if len(c.neg_zero):
        assert (bits(got[c.neg_zero]) == 0x80000000).all()
    if name == "none_valid":
        assert np.isinf(got).all() and (got < 0).any() and (got > 0).any()


# ---------------------------------------------------------------------------------------------- b. cost-only path
@pytest.fixture(scope="module")
def panda_handle(capi):
    from helpers import cfg_of
    from grasptrajopt_amd.robot_desc import load_builtin
    cfg = cfg_of("panda")
    h = capi.SolverHandle(load_builtin("panda"), cfg["link_ee"], cfg["link_gripper"], device=0)
    yield h
    h.close()


@pytest.mark.parametrize("half", ["mask", "obstacle_image"])
@pytest.mark.parametrize("sc", dc.scene_cases(), ids=lambda s: s.name)
def test_cost_only_fields_equal_oracle_at_the_voxel_centres(panda_handle, oracle_mod, sc, half):
    c, h = sc.case, panda_handle
    dobs = sc.depth_obstacle if half == "obstacle_image" else None
    shape, origin, bounds = h.scene_from_depth(0, c.depth, c.K, c.cam, target_mask=sc.target, threshold=c.threshold, grid_res=sc.grid_res,
                                               margin=sc.margin, epsilon=sc.epsilon, w_inside=sc.w_inside, depth_obstacle=dobs)
    assert_same_bits(bounds, dc.cloud_bounds(c), "bounds")
    q, want_shape = dc.voxel_centres(bounds, sc.margin, sc.grid_res)
    assert shape == want_shape and len(q) <= dc.MAX_VOXELS
    np.testing.assert_array_equal(origin, bounds[:, 0] - sc.margin)
    c_all, c_obs = h.scene_fields(0)
    args = (c.K, c.cam)
    _, sdf_a, in_a, want_all = oracle_field(oracle_mod, ("scene", sc.name, "all"), c.depth, *args, None, c.threshold, q, sc.epsilon, sc.w_inside)
    d2 = c.depth if dobs is None else dobs
    _, _, _, want_obs = oracle_field(oracle_mod, ("scene", sc.name, half), d2, *args, sc.target, c.threshold, q, sc.epsilon, sc.w_inside)
    assert_same_bits(c_all, want_all, "c_all")
    assert_same_bits(c_obs, want_obs, "c_obs")
    out = ~in_a
    assert (want_all[out] > 0).any() and (want_all[out] == 0).any()
    if sc.boundary:
        eps = np.float32(sc.epsilon)
        on = out & (np.abs(sdf_a.astype(np.float64) / float(eps) - 1.0) < 2e-7)
        assert on.sum() >= 2
        assert ((c_all[on] > 0) == (sdf_a[on] < eps)).all()


def test_scene_refuses_the_image_past_the_tree(capi, oracle_mod, panda_handle):
    c = dc.cases()["past_the_tree"]
    with pytest.raises(capi.GTOError, match=r"\(-4\): gto_scene_from_depth: image larger than 8192 x 4096 pixels"):
        panda_handle.scene_from_depth(1, c.depth, c.K, c.cam, threshold=c.threshold)
    w = dc.cases()["widest_tree"]  # the widest image it takes, and the handle serves it after the refusal
    shape, _, bounds = panda_handle.scene_from_depth(1, w.depth, w.K, w.cam, threshold=w.threshold, grid_res=0.2, margin=0.1)
    assert_same_bits(bounds, dc.cloud_bounds(w), "bounds")
    q, want_shape = dc.voxel_centres(bounds, 0.1, 0.2)
    assert shape == want_shape
    assert_same_bits(panda_handle.scene_fields(1)[0], oracle_mod.depth_sdf_cost(w.depth, w.K, w.cam, None, w.threshold, q)[3], "c_all")
    panda_handle.drop_scene(1)


# ---------------------------------------------------------------------------------------------- c. resident observation
@pytest.mark.parametrize("name", CASES)
def test_observation_sdf_and_check_posed_equal_oracle(capi, oracle_mod, monkeypatch, name):
    from grasptrajopt_amd.observation import Observation
    c = dc.cases()[name]
    _, sdf, inside, _ = oracle_of_case(oracle_mod, c)
    obs = Observation.from_depth(c.depth, c.K, c.cam, c.mask, c.threshold)
    for brute in ("0", "1"):
        monkeypatch.setenv("GTO_DEPTH_BRUTE", brute)
        got_sdf, got_in = obs.sdf(c.query)
        assert_same_bits(got_sdf, sdf, f"sdf (GTO_DEPTH_BRUTE={brute})")
        np.testing.assert_array_equal(got_in, inside)
    for n_points in dc.POSED_POINTS:
        pts, RT = dc.posed_instance(c, n_points)
        world = dc.placed(pts, np.nan_to_num(RT))
        ins = oracle_mod.depth_sdf_cost(c.depth, c.K, c.cam, c.mask, c.threshold, world.reshape(-1, 3))[2]
        want = ins.reshape(len(RT), n_points).sum(axis=1).astype(np.int32)
        want[2] = -1  # the NaN pose
        np.testing.assert_array_equal(obs.check_posed(pts, RT), want, err_msg=f"{n_points} points")
    obs.close()


# ---------------------------------------------------------------------------------------------- d. check_plans
@pytest.mark.parametrize("T", dc.PLAN_HORIZONS)
@pytest.mark.parametrize("name", dc.PLAN_ROBOTS)
def test_check_plans_on_a_depth_observation_equals_oracle(capi, oracle_mod, monkeypatch, name, T):
    from grasptrajopt_amd.observation import Observation
    desc, ee, gr, ngp = dc.plan_robot(name)
    opts = oracle_mod.reference_opts(T=T, standoff_offset=-max(2, T // 5))
    h = capi.SolverHandle(desc, ee, gr, opts, device=0, n_gripper_points=ngp)
    o = oracle_mod.Oracle(desc, ee, gr, opts, n_gripper_points=ngp)
    world_points = lambda q, base: o.eval_points(0, q, base, want_field=False)[0]
    inst = dc.plan_instance(name, desc, T, world_points)
    obs = Observation.from_depth(inst.depth, inst.K, inst.cam, None, inst.threshold)
    poisoned = inst.plans.copy()
    poisoned[inst.nan_at] = np.nan
    p, _, t = inst.nan_at
    for bases in (inst.base, inst.bases):
        want, n_undecided = dc.plan_expected(inst, desc, world_points, bases)
        assert n_undecided == 0
        assert (want == 0).any() and (want > 5).any() and want[p, t] == -1
        got = h.check_plans(obs, poisoned, bases)
        np.testing.assert_array_equal(got, want)
        clean = h.check_plans(obs, inst.plans, bases)  # the NaN changed nothing else
        assert clean[p, t] >= 0
        clean[p, t] = -1
        np.testing.assert_array_equal(clean, want)
        if T == 7:  # waypoints per workgroup: groups of 1, and of 3, 3 and 1
            for tg in ("1", "3"):
                monkeypatch.setenv("GTO_CHECK_TG", tg)
                np.testing.assert_array_equal(h.check_plans(obs, poisoned, bases), want, err_msg=f"GTO_CHECK_TG={tg}")
            monkeypatch.delenv("GTO_CHECK_TG")
    obs.close()
    h.close()
