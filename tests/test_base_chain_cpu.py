"""CPU: the restatement tests/test_gpu_base_chain.py compares the base placement chain with (tests/base_chain_ref.py) against
the reference's fixture and against BasePlanner's own formulation, the clearance that makes its collision counts exact on
every case the GPU file uses, and the draw assembly of BasePlanner.place_base."""
import numpy as np
import pytest

import base_chain_ref as ref
from conftest import golden


def test_restated_grid_and_offsets_equal_the_reference_fixture():
    d = golden("occupancy.npz")
    g = ref.grid(d["cloud"])
    np.testing.assert_array_equal(g.occupancy_grid_origin, d["origin"])
    assert tuple(g.occupancy_grid_shape) == tuple(d["shape"]) and g.occupancy_grid_size == int(d["size"])
    np.testing.assert_array_equal(g.occupancy_grid, d["grid"])
    np.testing.assert_array_equal(ref.offsets(g, d["query"]), d["offsets"])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_grid_point_sets_hold_what_they_are_chosen_for(n):
    p = ref.grid_points(n, seed=n)
    g = ref.grid(p)
    assert g.xlim_2d[1] == 1.3 and g.ylim_2d[1] == 0.9 and (n == 1 or g.ylim_2d[0] == -0.7)
    assert 0 < g.occupancy_grid.sum() < g.occupancy_grid_size
    if n >= 63:
        assert (p[:, 2] <= 0.01).any() and (p[:, 0] < -ref.MARGIN - ref.EPS).any()
        assert np.isnan(p[:, 2]).any() and np.isinf(p[:, 0]).any()
        # points on nodes mark their node; the ones epsilon away from a node are the restatement's to decide
        xg = g.xgrid
        on_node = [i for i in range(2, n) if i % 11 == 2 and p[i, 2] > 0.01 and np.abs(xg - p[i, 0]).min() == 0.0]
        assert on_node


@pytest.mark.parametrize("name,B,n_max,seed", ref.REPORT_CASES)
def test_report_cases_are_clear_of_cell_edges_and_count_like_base_collision_cost(oracle_mod, name, B, n_max, seed):
    desc, ee, gripper, ngp = ref.robot(name)
    orc = oracle_mod.Oracle(desc, ee, gripper, oracle_mod.reference_opts(), n_gripper_points=ngp)
    case = ref.report_case(orc, desc, B, n_max, seed)  # (asserts the clearance of every set)
    coll = ref.collisions(case.grid, case.foot, case.y, case.qc)
    for b in range(B):  # no set is left out: a case that fails here gets another seed
        placed = ref.place_by_inverse(case.foot[b], case.y[b])
        assert ref.clearance(case.grid, placed) >= ref.CLEARANCE, b
        assert ref.collision(case.grid, placed) == coll[b], b
    assert (B == 1 or ((coll > 0).any() and (coll == 0).any() if B > 100 else (coll > 0).any())) and case.n_goals[0] == n_max and (B == 1 or n_max == 1 or (case.n_goals < n_max).any())
    ep, er = ref.report(orc, desc.frame_index(ee), desc.frame_index(gripper), case.goals, case.n_goals, case.y, case.q)
    assert np.isnan(ep[case.n_goals[:, None] <= np.arange(n_max)]).all() and np.isfinite(ep[0]).all() and (er[0] > 1.0).any()


@pytest.mark.parametrize("name", sorted(ref.FIRST_FREE_PATTERNS))
def test_first_free_patterns(name):
    B, free, bad = ref.FIRST_FREE_PATTERNS[name]
    coll = ref.first_free_pattern(name)
    assert len(coll) == B and ref.first_free(coll) == (min(free) if free else -1)
    assert all(coll[b] == -1 for b in bad) and all(b < min(free) for b in bad)


@pytest.mark.parametrize("name", sorted(ref.FIRST_FREE_PATTERNS))
def test_first_free_scenes_are_clear_of_cell_edges_and_make_their_pattern(oracle_mod, name):
    desc, ee, gripper, ngp = ref.robot("fetch")
    orc = oracle_mod.Oracle(desc, ee, gripper, oracle_mod.reference_opts())
    sc = ref.first_free_scene(orc, name)  # (asserts the clearance of every finite set and the pattern of the counts)
    B, free, bad = ref.FIRST_FREE_PATTERNS[name]
    assert ref.first_free(sc.want) == ref.first_free(ref.first_free_pattern(name)) == (min(free) if free else -1)
    foot = ref.footprint(orc, sc.qc[:1])[0]
    for b in range(B):  # and in BasePlanner.base_collision_cost's formulation
        if b not in bad:
            placed = ref.place_by_inverse(foot, sc.y[b])
            assert ref.clearance(sc.grid, placed) >= ref.CLEARANCE and ref.collision(sc.grid, placed) == sc.want[b], b


def test_place_base_draws_are_the_drivers_concatenation():
    """examples/pybullet_gto_planning_mobile.py:163-181: `num` random rows of every object that has any, in object order."""
    from grasptrajopt_amd import BasePlanner
    rng = np.random.default_rng(2)
    objs = [rng.random((5, 4, 4)), np.zeros((0, 4, 4)), rng.random((3, 4, 4)), rng.random((1, 4, 4))]
    idx = rng.integers(0, 1, (6, 4, 2))
    for o, r in enumerate(objs):
        if len(r):
            idx[:, o] = rng.integers(0, len(r), (6, 2))
    sets, used = BasePlanner.draw_goal_sets(objs, indices=idx)
    assert sets.shape == (6, 6, 4, 4) and np.array_equal(used, idx)
    for d in range(6):
        want = np.concatenate([objs[o][idx[d, o]] for o in (0, 2, 3)])
        assert sets[d].tobytes() == want.tobytes()
    # sampled: every row comes from its object, in object order, and the indices that are returned rebuild the sets
    sets2, used2 = BasePlanner.draw_goal_sets(objs, num=3, draws=4, rng=np.random.default_rng(5))
    assert sets2.shape == (4, 9, 4, 4) and used2.shape == (4, 4, 3)
    again, _ = BasePlanner.draw_goal_sets(objs, indices=used2)
    assert again.tobytes() == sets2.tobytes()
    with pytest.raises(ValueError):
        BasePlanner.draw_goal_sets(objs, indices=idx[:, :3])
