"""tests/cloud_cases.py held to what it claims (no GPU): the stated trees, the zero extents, the ties (in lattice3d between
samples of different leaves at exactly the k-th distance), the restatement's own tie handling, the spread of the expected
counts of the two collision checks, and that no robot point of a plan instance lies within 1e-9 of a decision."""
import numpy as np
import pytest

import cloud_cases as cc
import cloud_sdf_ref as ref
import depth_cases as dc


def test_every_case_has_its_stated_tree_and_query_count():
    cs = cc.cases()
    assert list(cs) == list(cc.STATED_LEAVES)
    for name, c in cs.items():
        n = len(c.points)
        assert cc.leaf_slots(n) == cc.STATED_LEAVES[name], name
        assert c.points.shape == c.normals.shape and np.isfinite(c.points).all() and np.isfinite(c.normals).all()
        assert len(c.query) % 64 != 0 and set(c.ks) <= set(cc.KS) and n >= max(c.ks), name
    assert len(cs["n_equals_k_1"].query) == 1
    for k in cc.KS:
        assert len(cs[f"n_equals_k_{k}"].points) == k and cs[f"n_equals_k_{k}"].ks == (k,)
    # every compiled list at its first and its last k (GTO_CLOUD_DISPATCH: k <= 1, k <= 12, else)
    assert {1, 2, 12, 13, 16} <= set(cc.KS) and max(cc.KS) == cc.MAX_K
    assert len(cs["all_same"].points) > cc.MAX_K
    assert len(cs["leaf_shapes_32"].points) == cc.LEAF
    assert len(cs["scattered"].points) == 20000 and len(cs["scattered"].query) == 1000


def test_degenerate_clouds_are_degenerate():
    cs = cc.cases()
    for name, axes in cc.ZERO_EXTENT.items():
        p = cs[name].points
        ext = p.max(0) - p.min(0)
        assert (ext[list(axes)] == 0).all() and (np.delete(ext, list(axes)) > 0).all(), name
        key = cc.sample_keys(p)
        for a in axes:  # the axis adds nothing to any key
            assert (key & np.uint32(0x09249249 << a) == 0).all(), (name, a)
    assert len(np.unique(cs["all_same"].points, axis=0)) == 1 and (cc.sample_keys(cs["all_same"].points) == 0).all()
    nz = cs["all_same"].normals[:, 2]
    assert (nz[0::2] == 1).all() and (nz[1::2] == -1).all()
    # duplicates: sample c * 50 + j is copy c of point j; the copies of a point share a key and straddle a leaf border
    d = cs["duplicates"]
    assert len(np.unique(d.points, axis=0)) == 50 and (d.points.reshape(20, 50, 3) == d.points[:50]).all()
    leaf = cc.sample_leaves(d.points).reshape(20, 50)
    assert ((leaf.max(axis=0) - leaf.min(axis=0)) == 1).sum() >= 20
    assert not (d.normals.reshape(20, 50, 3)[0] == d.normals.reshape(20, 50, 3)[1]).all(axis=1).any()
    # far_apart: two key cells along x, and one leaf holds samples of both clusters
    f = cs["far_apart"]
    assert len(np.unique(cc.sample_keys(f.points) & np.uint32(0x09249249))) == 2
    leaf, right = cc.sample_leaves(f.points), f.points[:, 0] > 1.0
    assert any(right[leaf == l].any() and not right[leaf == l].all() for l in range(7))
    # collinear and coplanar are what they are called
    assert len(np.unique(cs["collinear"].points[:, 0])) == 300
    assert len(np.unique(np.round(cs["coplanar"].points[:, :2] * 64), axis=0)) == 1024
    # scattered: consecutive queries are far apart (sorted queries of this density would be about 0.1 apart)
    s = cs["scattered"]
    assert np.median(np.linalg.norm(np.diff(s.query, axis=0), axis=1)) > 0.5


@pytest.mark.parametrize("name", cc.TIE_CASES)
def test_tie_cases_tie_and_the_restatement_orders_ties_by_index(name):
    """knn_rows against a full stable argsort (= (value, index) order) on every case made for ties, and the k-th and (k+1)-th
    distances equal at some query for every k of the case."""
    c = cc.cases()[name]
    r = cc.squared_distances(c.points, c.query)
    full = np.argsort(r, axis=1, kind="stable")
    for k in c.ks:
        np.testing.assert_array_equal(ref.knn_rows(r, k), full[:, :k + 1], err_msg=f"k = {k}")
        e = cc.expected(name, k)
        np.testing.assert_array_equal(e["nearest"], full[:, 0])
        assert (e["d2"][:, k - 1] == e["d2"][:, k]).any(), (name, k)
    if name == "all_same":  # the k lowest indices win: the vote is that of samples 0 .. k - 1
        below, above = c.query[:, 2] < 0.5, c.query[:, 2] > 0.5
        for k in c.ks:
            e = cc.expected(name, k)
            np.testing.assert_array_equal(e["inside"][below], np.full(below.sum(), k % 2 == 1))
            assert not e["inside"][above].any() and e["nearest"].max() == 0


def test_lattice3d_ties_across_leaves_at_the_kth_distance():
    """For every k: at least a quarter of the queries tie at the k-th distance (the queries are nodes, face centres, cell
    centres and random points in equal parts, and for every k at least one of the first three kinds ties: shells of 1, 6, 12
    samples around a node, 4, 8 around a face centre, 8, 24 around a cell centre), and at some query the k-th and the
    (k+1)-th nearest sample, equally far, lie in different leaves of the sorted cloud.  The packet walk reaches one of the
    two leaves first; if it is the one of the (k+1)-th sample, the box of the other one is then AT the distance kth
    whenever the k-th sample is the box's nearest point to the query."""
    c = cc.cases()["lattice3d"]
    leaf = cc.sample_leaves(c.points)
    assert np.bincount(leaf).tolist() == [32] * 16
    assert not (np.diff(np.lexsort(c.points.T[::-1])) == 1).all()  # index order is not lattice order
    for k in cc.KS:
        e = cc.expected("lattice3d", k)
        idx = ref.knn_rows(cc.squared_distances(c.points, c.query), k)
        tie = e["d2"][:, k - 1] == e["d2"][:, k]
        assert tie.mean() >= 0.25, (k, tie.mean())
        cross = tie & (leaf[idx[:, k - 1]] != leaf[idx[:, k]])
        assert cross.any(), k
        assert (idx[cross, k - 1] < idx[cross, k]).all()


def test_lattice3d_has_queries_that_need_the_box_at_the_kth_distance():
    """The walk of one query alone, restated (cloud_cases.single_lane_walk): with `<=` in the skip tests it returns the
    restatement's neighbours on every query of lattice3d and every k; with `<` it returns others on the witnesses, every one
    of them a query whose k-th and (k+1)-th distances tie.  tests/test_gpu_cloud_cases.py asks the witnesses one per launch."""
    c = cc.cases()["lattice3d"]
    idx = np.argsort(cc.squared_distances(c.points, c.query), axis=1, kind="stable")
    witnesses = cc.lattice_witnesses()
    for k in cc.KS:
        for row in range(len(c.query)):
            assert cc.single_lane_walk(c.points, c.query[row], k) == idx[row, :k].tolist(), (k, row)
        e = cc.expected("lattice3d", k)
        assert len(witnesses[k]) >= 4 and (e["d2"][witnesses[k], k - 1] == e["d2"][witnesses[k], k]).all(), k


def test_nonfinite_queries_are_laid_out_as_stated():
    c = cc.cases()["leaf_shapes_257"]
    q, bad_at, finite_at, kinds = cc.nonfinite_queries(c)
    assert len(q) == 142 and len(q) % 64 != 0 and len(kinds) == len(bad_at)
    np.testing.assert_array_equal(q[finite_at], c.query[:130])
    for row, kind in zip(bad_at, kinds):
        assert np.isnan(q[row]).any() == (kind == "nan") and (kind == "nan" or np.isinf(q[row]).any())
    assert {0, 63, 64, 127, 128} <= set(bad_at.tolist())  # first and last lanes of waves (in the caller's order)


@pytest.mark.parametrize("sc", cc.scene_cases(), ids=lambda s: s.name)
def test_scene_grids_are_small_and_cost_something(sc):
    c = sc.case
    shape, origin, q = cc.planner_grid(c.points, sc.grid_res, sc.margin)
    assert len(q) <= cc.MAX_VOXELS < 40000 and sc.k <= sc.n_obstacle <= len(c.points)
    if c.name == "coplanar":  # the z axis is the margin alone
        assert shape[2] == len(np.arange(0.25 - sc.margin, 0.25 + sc.margin, sc.grid_res)) and c.points[:, 2].min() == c.points[:, 2].max()
    for n in (len(c.points), sc.n_obstacle):
        cost, inside = cc.scene_field(sc, n)
        assert (cost > 0).any() and (cost == 0).any() and inside.any() and not inside.all()
        assert (cost[~inside] > 0).any()  # the band 0 < sdf < epsilon is met
    if sc.n_obstacle == sc.k:  # (one sample fewer need not change a voxel: the last copy of a duplicated point never votes)
        assert (cc.scene_field(sc, sc.n_obstacle)[0] != cc.scene_field(sc, len(c.points))[0]).any()


@pytest.mark.parametrize("name", cc.POSED_CASES)
def test_posed_instances_count_some_and_not_all(name):
    for k in cc.POSED_KS:
        for P in dc.POSED_POINTS:
            pts, RT, want = cc.posed_counts(name, P, k)
            assert pts.shape == (P, 3) and RT.shape == (6, 4, 4) and want[2] == -1 and (np.delete(want, 2) >= 0).all()
            assert np.isnan(RT[2]).sum() == 1 and np.isfinite(np.delete(RT, 2, axis=0)).all()
            if P > 1:
                assert ((want > 0) & (want < P)).any(), (name, k, P, want)


def test_second_chunk_of_check_posed_is_one_pose():
    s = cc.CHUNK_POSED
    # chunk_items(n, P) = min(n, max(1, kCheckChunkQueries / P)) = 4096 poses; pose 4096 is the second chain
    assert cc.CHUNK_QUERIES // s.P == 4096 and s.n == 4097 and s.P * s.n == cc.CHUNK_QUERIES + s.P
    points, normals, pts, poses, want = cc.chunk_posed_instance()
    assert cc.leaf_slots(len(points)) == (2, 2) and pts.shape == (s.P, 3) and poses.shape == (s.n, 4, 4) and want.shape == (s.n,)
    assert (want[2::6] == -1).all() and (np.delete(want, np.arange(2, s.n, 6)) >= 0).all()
    assert 0 < want[4096] < s.P and len(set(want[:6].tolist())) >= 4
    np.testing.assert_array_equal(poses[4096], poses[4])


def test_undecided_marks_near_ties_and_near_zero_votes():
    k = 3
    d2 = np.array([[1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, (np.sqrt(3.0) + 5e-10) ** 2], [1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 4.0],
                   [1.0, 2.0, 3.0, 4.0]])
    dot = np.array([[-1.0, -1.0, 1.0], [-1.0, -1.0, 1.0], [-1.0, -1e-10, 1.0], [-1.0, 1e-10, 1.0], [-1.0, -1.0, -1e-10]])
    np.testing.assert_array_equal(cc.undecided({"d2": d2, "dot": dot}, k), [False, True, True, True, False])


# ------------------------------------------------------------------------------------------ plans against a box of samples
@pytest.fixture(scope="module")
def plan_oracles(oracle_mod):
    out = {}
    for name in dc.PLAN_ROBOTS:
        desc, ee, gr, ngp = dc.plan_robot(name)
        o = oracle_mod.Oracle(desc, ee, gr, n_gripper_points=ngp)
        out[name] = (desc, lambda q, base, o=o: o.eval_points(0, q, base, want_field=False)[0])
    return out


def test_pruned_restatement_equals_the_full_one(plan_oracles):
    """cloud_sdf_pruned against cloud_sdf, every output in its bits, on all points of two whole instances."""
    for name, T in (("panda", 5), ("random", 7)):
        desc, world_points = plan_oracles[name]
        inst = cc.plan_cloud(name, desc, T, world_points)
        q = inst.plans.transpose(0, 2, 1).reshape(dc.PLAN_B * T, desc.ndof)
        xyz = world_points(q, np.repeat(inst.bases, T, axis=0)).reshape(-1, 3)
        a, b = ref.cloud_sdf_pruned(inst.points, inst.normals, xyz, cc.PLAN_K), ref.cloud_sdf(inst.points, inst.normals, xyz, cc.PLAN_K)
        for key in b:
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
            np.testing.assert_array_equal(a[key].view(np.uint8), b[key].view(np.uint8), err_msg=key)


@pytest.mark.parametrize("T", dc.PLAN_HORIZONS)
@pytest.mark.parametrize("name", dc.PLAN_ROBOTS)
def test_plan_instances_have_no_undecided_point(plan_oracles, name, T):
    desc, world_points = plan_oracles[name]
    inst, want = cc.plan_case(name, T, desc, world_points)
    assert inst.plans.shape == (dc.PLAN_B, desc.ndof, T) and np.isfinite(inst.plans).all()
    # a closed box: sides of whole cells, one sample per cell, every sample on its face and within its cell, normals outward
    cells = np.rint((inst.hi - inst.lo) / cc.SPACING).astype(int)
    np.testing.assert_allclose(inst.lo + cells * cc.SPACING, inst.hi, atol=1e-12)
    assert len(inst.points) == 2 * (cells[0] * cells[1] + cells[1] * cells[2] + cells[2] * cells[0]) > 2 * cc.LEAF
    axis = np.abs(inst.normals).argmax(axis=1)
    assert (np.abs(inst.normals).sum(axis=1) == 1).all()
    face = np.where(inst.normals[np.arange(len(axis)), axis] > 0, inst.hi[axis], inst.lo[axis])
    assert (inst.points[np.arange(len(axis)), axis] == face).all()
    off = np.abs((inst.points - inst.lo) / cc.SPACING % 1.0 - 0.5) * cc.SPACING
    off[np.arange(len(axis)), axis] = 0.0
    assert off.max() <= cc.JITTER + 1e-12 and off.max() > 0.5 * cc.JITTER
    for counts, n_undecided in want.values():
        assert n_undecided == 0
        assert (counts == -1).sum() == 1 and counts[inst.nan_at[0], inst.nan_at[2]] == -1
    assert any((c > 0).any() for c, _ in want.values())


@pytest.mark.parametrize("name", dc.PLAN_ROBOTS)
def test_plan_counts_straddle_the_evaluators_threshold(plan_oracles, name):
    """Per robot, over its horizons and both base variants: a waypoint with no point inside, one with 1 to 5 and one with
    more than 5 (the evaluator calls a plan colliding at more than 5)."""
    desc, world_points = plan_oracles[name]
    counts = np.concatenate([c.reshape(-1) for T in dc.PLAN_HORIZONS for c, _ in cc.plan_case(name, T, desc, world_points)[1].values()])
    assert (counts == 0).any() and ((counts >= 1) & (counts <= 5)).any() and (counts > 5).any()


def test_second_chunk_of_check_plans_is_one_plan(plan_oracles):
    desc, _ = plan_oracles[cc.CHUNK_PLANS.robot]
    T, P = cc.CHUNK_PLANS.T, desc.n_points
    B = cc.chunk_plans_B(P, T)
    # chunk_items(B, T * P) = min(B, kCheckChunkQueries / (T * P)) = B - 1 plans; the last plan is the second chain
    assert T in dc.PLAN_HORIZONS and (B - 1) * T * P <= cc.CHUNK_QUERIES < B * T * P
