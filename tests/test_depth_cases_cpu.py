"""CPU: the instances of tests/depth_cases.py do what its text claims, by the FP64 oracle alone (no GPU).  The GPU side is
tests/test_gpu_depth_cases.py."""
import numpy as np
import pytest

import depth_cases as dc

NEG_ZERO = np.uint32(0x80000000)


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def oracle_of(oracle_mod, c, query=None, epsilon=None):
    return oracle_mod.depth_sdf_cost(c.depth, c.K, c.cam, c.mask, c.threshold, c.query if query is None else query,
                                     epsilon=c.epsilon if epsilon is None else epsilon, w_inside=c.w_inside)


def test_every_case_has_its_stated_hierarchy_and_query_count():
    cs = dc.cases()
    assert list(cs) == list(dc.STATED_P)
    for name, c in cs.items():
        assert c.P == dc.STATED_P[name], name
        assert c.depth.dtype == np.float32 and c.query.shape[1] == 3
    assert cs["widest_tree"].P == dc.MAX_P and cs["past_the_tree"].P == 2 * dc.MAX_P
    nq = sorted(len(c.query) for c in cs.values())
    assert set(nq) >= {1, 63, 64, 65, 255, 256, 257} and 2000 <= nq[-1] <= 4000
    # the strips: all but one row or column of leaf slots empty
    assert cs["row_strip"].depth.shape == (1, 200) and cs["col_strip"].depth.shape == (130, 1)


@pytest.mark.parametrize("name", list(dc.STATED_P))
def test_restatements_equal_the_oracle_and_the_queries_are_what_they_claim(oracle_mod, name):
    c = dc.cases()[name]
    pts, sdf, inside, cost = oracle_of(oracle_mod, c)
    mine, valid = dc.backproject(c.depth, c.K, c.cam, c.mask, c.threshold)
    np.testing.assert_array_equal(mine[valid], pts)  # the same bits: a query put on a point is at distance 0
    p = dc.project(c.depth, c.K, c.cam, c.query)
    np.testing.assert_array_equal(p.inside, inside)
    if name == "none_valid":
        assert len(pts) == 0 and np.isinf(sdf).all() and inside.any() and (~inside).any()
        return
    assert len(pts) == {"single_valid": 1, "one_pixel": 1}.get(name, len(pts)) and len(pts) > 0
    # queries on cloud points: distance 0, and -0.0 where the visibility test says inside
    assert len(c.on_cloud) and len(c.neg_zero)
    assert (sdf[c.on_cloud] == 0).all()
    assert inside[c.neg_zero].all() and (bits(sdf[c.neg_zero]) == NEG_ZERO).all()
    plus = np.setdiff1d(c.on_cloud, c.neg_zero)
    assert (bits(sdf[plus]) == 0).all()
    if len(c.query) > 1:  # (the one query of the nq = 1 case is the -0.0 one)
        assert inside.any() and (~inside).any()
        # pixel coordinates in (-1, 0) that truncation puts into the image
        assert (p.in_view & ((p.ux < 0) | (p.uy < 0))).any()
    if len(c.query) >= 64:
        assert (np.abs(c.query).max(axis=1) >= 1.0e6).sum() >= 4
        assert (cost > 0).any()


def test_degenerate_clouds_are_degenerate(oracle_mod):
    cs = dc.cases()
    flat = oracle_of(oracle_mod, cs["flat_wall"])[0]
    assert np.ptp(flat[:, 2]) == 0.0 and np.ptp(flat[:, 0]) > 0 and np.ptp(flat[:, 1]) > 0  # z extent exactly 0
    p = dc.project(cs["flat_wall"].depth, cs["flat_wall"].K, cs["flat_wall"].cam, cs["flat_wall"].query)
    z0 = p.pc_z == 0.0
    assert z0.sum() == 8 and not p.in_view[z0].any() and np.isnan(p.ux[z0]).sum() == 1 and np.isinf(p.ux[z0]).sum() >= 6
    holes = cs["holes"]
    _, valid = dc.backproject(holes.depth, holes.K, holes.cam, holes.mask, holes.threshold)
    v = valid.reshape(holes.depth.shape)
    tiles = [(cy, cx) for cy in range(9) for cx in range(9) if not v[4 * cy:4 * cy + 4, 8 * cx:8 * cx + 8].any()]
    assert len(tiles) >= 14 and v[18, 27] and v[16:24, 24:40].sum() == 1
    assert not v[:, 52:55].any() and (holes.depth[:, 52:55] > holes.threshold).all()
    sv = cs["single_valid"]
    assert dc.backproject(sv.depth, sv.K, sv.cam, sv.mask, sv.threshold)[1].sum() == 1
    assert sv.mask is None and (sv.depth == 0).any() and (sv.depth > sv.threshold).any()
    nv = cs["none_valid"]
    assert (nv.depth == 0).any() and (nv.depth > nv.threshold).any() and ((nv.mask == 1) & (nv.depth > 0) & (nv.depth < nv.threshold)).any()


# ------------------------------------------------------------------------------------------ workspace grids
@pytest.mark.parametrize("sc", dc.scene_cases(), ids=lambda s: s.name)
def test_scene_grids_are_small_and_cost_something(oracle_mod, sc):
    c = sc.case
    q, shape = dc.voxel_centres(dc.cloud_bounds(c), sc.margin, sc.grid_res)
    assert 0 < len(q) <= dc.MAX_VOXELS, shape
    _, sdf, inside, cost = oracle_mod.depth_sdf_cost(c.depth, c.K, c.cam, None, c.threshold, q, epsilon=sc.epsilon, w_inside=sc.w_inside)
    out = ~inside
    assert (cost[out] > 0).any() and (cost[out] == 0).any()  # the search's early bound has voxels to cut and voxels to keep
    if not sc.boundary:
        return
    eps = np.float32(sc.epsilon)
    assert eps == np.float32(sc.grid_res) and abs(sc.margin / sc.grid_res - 3) < 1e-12
    # voxel centres on the boundary dist < epsilon to within rounding, as the oracle evaluates it ...
    on = out & (np.abs(sdf.astype(np.float64) / float(eps) - 1.0) < 2e-7)
    assert on.sum() >= 2, on.sum()
    # ... and on both sides of it
    assert (sdf[out] < eps).any() and (sdf[out] >= eps).any()
    if sc.name == "single_valid_boundary":  # six face neighbours of the point's voxel: rounding alone decides
        assert on.sum() >= 6 and (sdf[on] < eps).any() and (sdf[on] >= eps).any(), (on.sum(), sdf[on])
        assert ((cost[on] > 0) == (sdf[on] < eps)).all()


# ------------------------------------------------------------------------------------------ plans through an image
@pytest.fixture(scope="module")
def plan_oracles(oracle_mod):
    out = {}
    for name in dc.PLAN_ROBOTS:
        desc, ee, gr, ngp = dc.plan_robot(name)
        o = oracle_mod.Oracle(desc, ee, gr, n_gripper_points=ngp)
        out[name] = (desc, lambda q, base, o=o: o.eval_points(0, q, base, want_field=False)[0])
    return out


@pytest.mark.parametrize("T", dc.PLAN_HORIZONS)
@pytest.mark.parametrize("name", dc.PLAN_ROBOTS)
def test_plan_instances_have_no_undecided_point(plan_oracles, name, T):
    desc, world_points = plan_oracles[name]
    inst = dc.plan_instance(name, desc, T, world_points)
    assert inst.plans.shape == (dc.PLAN_B, desc.ndof, T) and np.isfinite(inst.plans).all()
    for bases in (inst.base, inst.bases):
        counts, n_undecided = dc.plan_expected(inst, desc, world_points, bases)
        assert n_undecided == 0
        assert (counts == 0).any() and (counts > 5).any(), counts
        assert (counts == -1).sum() == 1
    if name == "random":
        assert (desc.joint_type[[f for f in range(desc.n_frames) if desc.q_index[f] in set(desc.opt_index.tolist())]] == 2).any()
