"""CPU: the small-robot cases of tests/small_robots.py are what their names promise, the FP64 oracle solves every one of them
(trajectory, IK, base placement) to an ordinary end, and no decision of those solves sits on round-off, so that
tests/test_gpu_small_robots.py may compare iteration counts for equality.  The restatements the GPU file compares the other
entry points with (ik_pose_ref, retime_ref, depth_cases, cloud_cases) are checked on the same inputs."""
import numpy as np
import pytest

import small_robots as sr

# kind -> frames, ndof, n_opt, links, points (None: 3 to 9 per link), gripper points, links an optimised joint moves
PROMISED = {
    "chain_1": (2, 1, 1, 2, None, 3, 1), "chain_2": (3, 2, 2, 3, None, 3, 2), "chain_3": (4, 3, 3, 4, None, 3, 3),
    "chain_4": (5, 4, 4, 5, None, 3, 4), "chain_5": (6, 5, 5, 6, None, 3, 5), "chain_6": (7, 6, 6, 7, None, 3, 6),
    "chain_7": (8, 7, 7, 8, None, 3, 7), "chain_9_short": (10, 9, 9, 10, None, 3, 9), "one_point": (2, 1, 1, 1, 1, 1, 1),
    "static_links_only": (2, 1, 1, 1, 5, 3, 0), "prismatic_only": (3, 2, 2, 3, 12, 3, 2), "ee_above_joints": (4, 3, 3, 4, 15, 3, 3),
    "ee_not_gripper": (4, 2, 2, 4, 15, 3, 3), "root_joint": (1, 1, 1, 1, 5, 3, 1),
}
CASES = sr.case_ids()


@pytest.fixture(scope="module")
def solved(oracle_mod):
    """case id -> (case, oracle), built once."""
    made = {}

    def get(cid):
        if cid not in made:
            c = sr.Case(oracle_mod, *cid)
            made[cid] = (c, c.oracle(oracle_mod))
        return made[cid]
    return get


def test_no_kind_left_the_list():
    assert sorted(sr.KINDS) == sorted(PROMISED) and len(set(sr.KINDS)) == len(sr.KINDS)
    ids = set(CASES)
    for kind in sr.KINDS:
        assert {(kind, 4, (5, 5, 5)), (kind, 5, (5, 5, 5))} <= ids
    for kind in ("chain_1", "one_point", "static_links_only"):
        assert (kind, 50, (5, 5, 5)) in ids
    for kind in ("one_point", "chain_2"):
        assert {(kind, T, s) for T in (4, 5) for s in ((1, 1, 1), (1, 4, 1))} <= ids
    assert sr.HORIZONS == {4: -1, 5: -2, 50: -10} and sr.B <= 6
    assert set(sr.RAGGED_KINDS) == {"chain_1", "chain_4", "one_point"} and sr.N_MAX == 3
    assert set(sr.RETIME_KINDS) == {"chain_1", "chain_2", "one_point"} and set(sr.RETIME_SUBDIVS) == {1, 2, 5}
    assert all(0 <= s < 20 for s in sr.SEEDS.values()) and set(sr.SEEDS) <= ids


@pytest.mark.parametrize("kind", list(PROMISED))
def test_kind_has_the_counts_its_name_promises(kind):
    for seed in {0} | {s for cid, s in sr.SEEDS.items() if cid[0] == kind}:
        r = sr.Robot(kind, seed=seed)
        d = r.desc
        frames, ndof, n_opt, links, points, ngp, moving = PROMISED[kind]
        got = r.counts()
        assert (got["frames"], got["ndof"], got["n_opt"], got["links"], got["gripper_points"], got["moving"]) == \
            (frames, ndof, n_opt, links, ngp, moving), got
        per_link = np.bincount(d.point_link, minlength=d.n_links)
        if points is None:
            assert per_link.min() >= 3 and per_link.max() <= 9
        else:
            assert got["points"] == points
        assert len(d.param_index) == 0 and d.opt_index.tolist() == list(range(ndof))   # no parameter joint
        assert (d.lower < 0).all() and (d.upper > 0).all()
        jt = d.joint_type.tolist()
        if kind.startswith("chain_"):
            assert d.parent.tolist() == list(range(-1, frames - 1)) and jt[0] == 0 and all(t != 0 for t in jt[1:])
            assert d.link_frame.tolist() == list(range(frames)) and r.ee == r.gripper == d.frame_names[-1]
        if kind == "one_point":
            assert d.link_frame.tolist() == [1] and d.link_is_moving().tolist() == [True]
        if kind == "static_links_only":
            assert d.link_frame.tolist() == [0] and d.link_is_moving().tolist() == [False]   # the PbChunk table is empty
            assert jt == [0, 1] and r.gripper == "f0"
        if kind == "prismatic_only":
            assert jt == [0, 2, 2]
        if kind == "ee_above_joints":
            assert jt == [0, 1, 1, 1] and r.ee == r.gripper == d.frame_names[0] and d.parent.tolist() == [-1, 0, 1, 2]
        if kind == "ee_not_gripper":
            assert jt == [0, 1, 1, 0] and (r.ee, r.gripper) == ("f2", "f3") and d.parent[3] == 2
        if kind == "root_joint":
            assert jt == [1] and d.parent.tolist() == [-1] and d.q_index.tolist() == [0] and np.abs(d.origin_xyz[0]).max() > 0


@pytest.mark.parametrize("cid", CASES, ids=sr.case_name)
def test_oracle_solves_the_case_and_no_decision_sits_on_round_off(solved, cid):
    """Trajectory, IK (with and without the scene) and base placement: finite cost, status CONVERGED or MAX_ITER, and the
    same iterations, statuses and results (1e-9) with every seed entry and goal translation moved by a relative 1e-12."""
    c, o = solved(cid)
    assert c.B <= 6 and c.Q0.shape == (c.B, c.desc.ndof, c.T) and np.abs(c.base).min() > 0
    d = c.desc
    assert (c.qg >= d.lower).all() and (c.qg <= d.upper).all() and (c.qc >= d.lower).all() and (c.qc <= d.upper).all()
    assert sr.robust_failures(c, o) == []
    if c.kind in sr.RAGGED_KINDS:
        assert sorted(set(c.n_goals_ragged.tolist())) == [1, 2, 3]
        assert sr.robust_failures(c, o, ragged=True) == []
    # the solves do something
    runs = dict((name, a) for name, a, _ in sr.robust_runs(c, o))
    assert (runs["solve_batch"][2] >= 2).all()
    # some surface points meet voxels that cost something, in both fields
    for use_obs in (False, True):
        val = o.eval_points(0, np.concatenate([c.Q0[b].T for b in range(c.B)]), np.repeat(c.base, c.T, axis=0), use_obs=use_obs)[2]
        assert (val > 0).any()
    assert c.scene[2] == cid[2]
    if max(cid[2]) < 5:  # the one voxel (or the two middle ones) holds the robot at every waypoint, base included
        xyz = o.eval_points(0, np.concatenate([c.Q0[b].T for b in range(c.B)]), np.repeat(c.base, c.T, axis=0))[0].reshape(-1, 3)
        u = (xyz - np.asarray(c.scene[3])) / c.scene[4]
        assert (u > 0).all() and (u < np.asarray(cid[2])).all()


@pytest.mark.parametrize("T", [4, 5])
def test_ee_above_joints_has_goal_blocks_of_exact_zeros(solved, T):
    c, o = solved(("ee_above_joints", T, (5, 5, 5)))
    Q = o.solve_batch(*c.solve_args())[0]
    for traj in (c.Q0, Q):
        _, _, _, Hg, gg = o.eval_normal_eq(0, c.goals, c.n_goals, c.S, c.base, traj)
        assert not Hg.any() and not gg.any()
        fg = o.eval_objective(0, c.goals, c.n_goals, c.S, c.base, traj)[0]
        assert (fg > 1e-4).all()     # the goals lie beside the root: the term is there, and no joint can change it
    assert o.eval_objective(0, c.goals, c.n_goals, c.S, c.base, Q)[0].tobytes() == o.eval_objective(0, c.goals, c.n_goals, c.S, c.base, c.Q0)[0].tobytes()
    # the base counterpart: a joint that moves no goal frame is damped by lambda itself (as in the IK solve), and the base is placed
    y, q, f, it, st = o.solve_base_batch(c.qc, c.goals, c.n_goals, 0.01, max_iter=sr.BASE_MAX_ITER)
    assert (st == 0).all() and (it >= 2).all() and np.abs(y).max() > 1e-3
    assert q[:, 0].tobytes() == c.qc.tobytes()


@pytest.mark.parametrize("T", [4, 5, 50])
def test_static_links_only_has_obstacle_blocks_of_exact_zeros(solved, T):
    c, o = solved(("static_links_only", T, (5, 5, 5)))
    Q = o.solve_batch(*c.solve_args())[0]
    f_obs = []
    for traj in (c.Q0, Q):
        A, g, ss = o.eval_obstacle_normal_eq(0, c.base, traj)
        assert not A.any() and not g.any() and (ss[:, 2:] > 0).all()
        f_obs.append(o.eval_objective(0, c.goals, c.n_goals, c.S, c.base, traj)[1])
        assert (f_obs[-1] > 0).all()
    assert f_obs[0].tobytes() == f_obs[1].tobytes()   # constant: no joint moves a point


def _pose_restatement_is_stable(solved, cid):
    """tests/ik_pose_ref.py on the cases' goals as quaternion and roll-pitch-yaw goals: a regular end, and the same
    iterations and statuses with the end effector's frame turned by +-1e-13 about each axis (ik_pose_cases.unstable)."""
    import ik_pose_cases as ipc
    import ik_pose_ref as ref
    c, o = solved(cid)
    for gk in (ref.GTO_IK_GOAL_QUATERNION, ref.GTO_IK_GOAL_RPY):
        q, f, it, st = sr.pose_restatement(c, o, gk)
        assert np.isfinite(f).all() and np.isin(st, (0, 1)).all()
        for Rt in ref.small_rotations(ipc.ETA):
            q2, f2, it2, st2 = sr.pose_restatement(c, o, gk, rot=Rt)
            assert np.array_equal(it, it2) and np.array_equal(st, st2) and np.abs(q - q2).max() <= 1e-9


@pytest.mark.parametrize("T", [4, 5])
@pytest.mark.parametrize("kind", sr.IK_KINDS)
def test_pose_ik_restatement_keeps_its_path_under_turned_frames(solved, kind, T):
    _pose_restatement_is_stable(solved, (kind, T, (5, 5, 5)))


@pytest.mark.parametrize("cid", [cid for cid in CASES if cid[0] in sr.IK_KINDS and (cid[1] == 50 or cid[2] != (5, 5, 5))], ids=sr.case_name)
def test_pose_ik_restatement_keeps_its_path_at_the_long_horizon_and_in_flat_fields(solved, cid):
    _pose_restatement_is_stable(solved, cid)


@pytest.mark.parametrize("T", [4, 5])
@pytest.mark.parametrize("kind", sr.RETIME_KINDS)
def test_retiming_inputs_have_converged_profiles(kind, T):
    import retime_ref as rr
    d, plans, vm, am = sr.retime_inputs(kind, T)
    assert plans.shape == (sr.RETIME_B, d.ndof, T) and d.ndof in (1, 2)
    assert (plans[1, 0] == plans[1, 0, 0]).all() and plans[3].tobytes() == plans[2][:, ::-1].tobytes()
    for subdiv in sr.RETIME_SUBDIVS:
        r = rr.retime(plans, vm, am, subdiv, 16)
        assert (r["status"] == 0).all() and np.isfinite(r["q"]).all()
        moving = np.any(plans != plans[:, :, :1], axis=(1, 2))
        assert moving.tolist() == [True, d.ndof > 1, True, True, True]
        assert (r["duration"][moving] > 0).all() and (r["duration"][~moving] == 0).all()


@pytest.mark.parametrize("T", [4, 5])
@pytest.mark.parametrize("kind", sr.RETIME_KINDS)
def test_retiming_inputs_have_certified_convex_profiles(kind, T):
    """tests/retime_convex_ref.py on the same plans, down to two variables (T = 4, subdiv = 1): every moving plan is solved
    within the Newton bound the GPU test holds the kernel to, and is never slower than the greedy profile; the plan without
    a moving joint takes no step."""
    import retime_convex_ref as cr
    import retime_ref as rr
    d, plans, vm, am = sr.retime_inputs(kind, T)
    moving = np.any(plans != plans[:, :, :1], axis=(1, 2))
    for subdiv in sr.RETIME_SUBDIVS:
        with np.errstate(divide="ignore", invalid="ignore"):
            r = cr.retime_paths_convex_ref(plans, None, vm, am, subdiv, 16, 1e-8)
        greedy = rr.retime(plans, vm, am, subdiv, 16)
        assert (r["status"] == 0).all() and np.isfinite(r["q"]).all()
        assert (r["iters"][moving] > 0).all() and (r["iters"] <= cr.MAX_NEWTON // 2).all() and (r["iters"][~moving] == 0).all()
        assert (r["duration"][~moving] == 0).all() and (r["duration"][moving] > 0).all()
        assert (r["duration"] <= greedy["duration"] * (1 + 1e-8)).all()


@pytest.mark.parametrize("T", [4, 5])
@pytest.mark.parametrize("kind", sr.RETIME_KINDS)
def test_torque_retiming_inputs_are_what_the_gpu_test_takes_them_for(kind, T):
    """tests/retime_torque_ref.py on sr.retime_torque_inputs: every joint of every kind feels gravity (a finite limit each:
    no kind is the convex call in disguise), every path is solved or INFEASIBLE, at least two are solved, and the plan that
    stands still is held exactly where sr.RETIME_STILL_HELD says -- chain_1 at T = 5 at no factor of the rule."""
    import dynamics_ref as dr
    import retime_convex_ref as cr
    import retime_torque_ref as tr
    for subdiv in sr.RETIME_SUBDIVS:
        d, fee, plans, vm, am, tm, pl = sr.retime_torque_inputs(kind, T, subdiv)
        assert d.has_inertials and np.isfinite(tm).all() and (tm > 0).all() and tm.shape == (d.ndof,)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = tr.retime_paths_torque_ref(d, fee, plans, None, vm, am, tm, pl, subdiv, 16, 1e-8)
            convex = cr.retime_paths_convex_ref(plans, None, vm, am, subdiv, 16, 1e-8)
        ok = r["status"] == 0
        assert np.isin(r["status"], (0, tr.GTO_STATUS_INFEASIBLE)).all() and ok.sum() >= 2
        assert (r["duration"][ok] >= convex["duration"][ok] * (1 - 1e-8)).all()
        if d.ndof == 1:
            assert bool(ok[1]) == sr.RETIME_STILL_HELD[kind, T] and r["iters"][1] == 0
            z = np.zeros(1)
            g = abs(dr.inverse_dynamics(d, plans[1][:, 0], z, z, fee, tr.payload_of(pl, 1))[0])
            if ok[1]:
                assert r["duration"][1] == 0 and np.allclose(np.abs(r["tau"][1]), g, rtol=1e-12) and g < tm[0]
            else:  # out of the rule's reach: 3 times the unloaded robot's largest static torque does not hold it
                top = max(np.abs(np.array([dr.inverse_dynamics(d, qi, z, z, fee) for qi in tr.path_points(p, subdiv)[0]])).max() for p in plans)
                assert g > 3.0 * top


def _plan_instances_are_decided(solved, cid):
    """The depth image and the sampled box that check_plans is run through: no surface point of the oracle within 1e-9 m of a
    decision, under the shared base and under the per-plan bases, and counts that are not all alike."""
    import cloud_cases as cc
    import depth_cases as dc
    kind, T = cid[:2]
    c, o = solved(cid)
    inst, world_points = sr.plan_depth_instance(c, o)
    assert inst.depth.shape == (60, 80) and inst.plans.shape == (dc.PLAN_B, c.desc.ndof, T)
    for bases in (inst.base, inst.bases):
        want, n_undecided = dc.plan_expected(inst, c.desc, world_points, bases)
        assert n_undecided == 0
        assert (want == 0).any() and want[inst.nan_at[0], inst.nan_at[2]] == -1 and want.max() <= c.desc.n_points
        # (the image hugs the first half of the motion from behind; where no joint moves a point, the second half is the first)
        assert (want > 0).any() == (kind != "static_links_only")
    inst, world_points = sr.plan_cloud_instance(c, o)
    both = []
    for bases in (inst.base, inst.bases):
        want, n_undecided = cc.plan_expected(inst, c.desc, world_points, bases)
        assert n_undecided == 0
        both.append(want)
    both = np.concatenate(both)
    assert (both > 0).any() and len(np.unique(both[both >= 0])) > 1   # (the box is 8 cm wide at the least: some of these robots never leave it)
    if kind == "one_point":
        assert c.desc.n_points == 1 and both.max() == 1


@pytest.mark.parametrize("T", [4, 5])
@pytest.mark.parametrize("kind", sr.PLAN_KINDS)
def test_plan_instances_have_no_undecided_point(solved, kind, T):
    _plan_instances_are_decided(solved, (kind, T, (5, 5, 5)))


@pytest.mark.parametrize("kind", sr.LONG_KINDS)
def test_plan_instances_at_the_long_horizon_have_no_undecided_point(solved, kind):
    _plan_instances_are_decided(solved, (kind, 50, (5, 5, 5)))


def test_every_kind_and_horizon_has_plan_instances():
    assert sorted(sr.plan_case_ids()) == sorted(cid for cid in CASES if cid[2] == (5, 5, 5)) and set(sr.PLAN_KINDS) == set(sr.KINDS)


IK_CASES = [cid for cid in CASES if cid[0] in sr.IK_KINDS]


@pytest.mark.parametrize("cid", IK_CASES, ids=sr.case_name)
def test_seed_choice_ties_are_the_recorded_ones(solved, cid):
    """The instances tests/test_gpu_small_robots.py leaves out of the comparison of the seed choice with the oracle's: the
    recorded number of exact cost ties, for float32 and float64 solutions alike, and never the instance whose rows all count."""
    from test_gpu_seed_waves import clearly_first, oracle_seeds
    c, o = solved(cid)
    c.o, c.offset = o, sr.HORIZONS[c.T]
    case = sr.seed_goalset_case(c)
    assert set(sr.SEED_TIES) <= set(IK_CASES) and all(1 <= n <= 3 for n in sr.SEED_TIES.values())
    for f32 in (True, False):
        want = oracle_seeds(c, case, f32)
        assert [w["n_accepted"] for w in want] == [5, 0, 5, 2]
        assert sr.seed_cost_ties(want) == sr.SEED_TIES.get(cid, 0)
        unclear = sum(not clearly_first(w["seed_cost"], w["oracle_dist"]) for w in want if w["n_accepted"])
        assert unclear <= 1 + sr.SEED_TIES.get(cid, 0)


@pytest.mark.parametrize("cid", [cid for cid in IK_CASES if cid[1] != 50], ids=sr.case_name)
def test_base_report_cases_are_clear_and_mixed(solved, cid):
    """base_chain_ref.report_case at the recorded seed: its own clearance assertion holds, and the restated footprint counts
    have both a colliding and a free set (the first free set is then neither 0 by default nor -1)."""
    import base_chain_ref as bref
    c, o = solved(cid)
    case = sr.base_report_case(c, o)
    assert case.q.shape == (sr.REPORT_B, sr.REPORT_N_MAX, c.desc.ndof) and case.n_goals[0] == sr.REPORT_N_MAX
    for b in range(sr.REPORT_B):
        assert bref.clearance(case.grid, bref.place(case.foot[b], case.y[b])) >= bref.CLEARANCE
    col = bref.collisions(case.grid, case.foot, case.y, case.qc)
    assert (col == 0).any() and (col > 0).any() and col.max() <= c.desc.n_points
