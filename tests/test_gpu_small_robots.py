"""GPU: every entry point on the smallest robots include/gto_solver.h accepts (tests/small_robots.py: chains of 1 to 7 joints,
the shortest 9-joint chain, one surface point, no moving link, prismatic joints only, an end effector above every joint, a
gripper that is not the end effector, a joint on the root frame), at T = 4, 5 and 50, in 5 x 5 x 5, 1 x 1 x 1 and 1 x 4 x 1
fields, against the FP64 oracle (oracle/gto_oracle.c) and the numpy restatements, at the tolerances tests/test_gpu_limits.py,
tests/test_gpu_parity.py and the suites of the other entry points hold the large robots to.  tests/test_small_robots_cpu.py
shows on the CPU that no decision of the oracle's solves of these cases sits on round-off, so iteration counts are compared
for equality.  No call has more than 6 instances.  Run the file under a time limit and stop at the first fault:
timeout -k 10 600 pytest -x tests/test_gpu_small_robots.py."""
import numpy as np
import pytest

import base_chain_ref as bref
import cloud_cases as cc
import depth_cases as dc
import grasp_chain_ref as gref
import ik_pose_ref as pref
import small_robots as sr
from helpers import exhaustive

pytestmark = pytest.mark.gpu

CASES = sr.case_ids()
IK_CASES = [cid for cid in CASES if cid[0] in sr.IK_KINDS]   # the IK and base kernels take up to eight optimised joints
REPORT_CASES = [cid for cid in IK_CASES if cid[1] != 50]     # gto_base_report_device reads no horizon: the T = 4 and 5 handles
PLAN_CASES = sr.plan_case_ids()                              # every kind at every horizon of the kind
OK = (0, 1)  # GTO_STATUS_CONVERGED, GTO_STATUS_MAX_ITER


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def rigs(capi, oracle_mod):
    """case id -> the case with its oracle (.o), its handle (.h) and what tests/test_gpu_seed_waves.check_seeds reads of a rig."""
    made = {}

    def get(cid):
        if cid not in made:
            c = sr.Case(oracle_mod, *cid)
            c.o, c.h, c.offset = c.oracle(oracle_mod), c.handle(capi), sr.HORIZONS[c.T]
            c.nt = c.o.usable_cores()
            made[cid] = c
        return made[cid]
    yield get
    for c in made.values():
        c.h.close()


# ------------------------------------------------------------------------------------------------- evaluation
@pytest.mark.parametrize("cid", CASES, ids=sr.case_name)
def test_pieces_match_oracle(rigs, oracle_mod, cid):
    c = rigs(cid)
    d, h, o = c.desc, c.h, c.o
    rng = np.random.default_rng(3)
    q = rng.uniform(d.lower, d.upper, size=(6, d.ndof))
    np.testing.assert_allclose(h.eval_fk(q), o.eval_fk(q), rtol=0, atol=1e-12)
    qs = np.concatenate([c.Q0[0].T[::9], c.qc])[:6]
    for use_obs in (False, True):
        xg, og, vg, gg = h.eval_points(0, qs, c.base[0], use_obs=use_obs)
        xo, oo, vo, go = o.eval_points(0, qs, c.base[0], use_obs=use_obs)
        np.testing.assert_allclose(xg, xo, rtol=0, atol=1e-12)
        np.testing.assert_array_equal(og, oo)
        np.testing.assert_array_equal(vg, vo)
        hg = h.eval_points_hessian(0, qs, c.base[0], use_obs=use_obs)
        fld = c.scene[1] if use_obs else c.scene[0]
        _, _, ho = oracle_mod.sdf_eval(fld, c.scene[2], c.scene[3], c.scene[4], xo.reshape(-1, 3))
        np.testing.assert_array_equal(hg.reshape(-1, 3, 3), ho)
    for goals, ng in ((c.goals, c.n_goals), (c.goals_all, c.n_goals_ragged)):
        for S in (c.S, None):
            a = h.eval_objective(0, goals, ng, S, c.base, c.Q0)
            b = o.eval_objective(0, goals, ng, S, c.base, c.Q0)
            for x, y in zip(a[:3], b[:3]):
                np.testing.assert_allclose(x, y, rtol=1e-9, atol=1e-13)
            np.testing.assert_array_equal(a[3], b[3])
    A, g, ss = h.eval_obstacle_normal_eq(0, c.base, c.Q0)
    Ao, go, sso = o.eval_obstacle_normal_eq(0, c.base, c.Q0)
    assert sso.max() > 0
    np.testing.assert_allclose(A[:, 2:], Ao[:, 2:], rtol=1e-8, atol=1e-10 * max(np.abs(Ao).max(), 1e-30))
    np.testing.assert_allclose(g[:, 2:], go[:, 2:], rtol=1e-8, atol=1e-10 * max(np.abs(go).max(), 1e-30))
    np.testing.assert_allclose(ss, sso, rtol=1e-11, atol=1e-15)
    if c.kind == "static_links_only":  # no optimised joint moves a point: blocks of exact zeros, a constant f_obs > 0
        assert not A[:, 2:].any() and not g[:, 2:].any() and (ss[:, 2:] > 0).all()
    for b in range(c.B):
        cg, dg = h.plan_cost(0, c.Q0, c.base[b])
        co, do = o.plan_cost(0, c.Q0, c.base[b])
        np.testing.assert_allclose(cg, co, rtol=1e-12)
        np.testing.assert_allclose(dg, do, rtol=1e-14)


# ------------------------------------------------------------------------------------------------- the trajectory solve
def _solve_against_oracle(capi, monkeypatch, c, ragged):
    args = c.solve_args(ragged)
    Qg, dQg, fg, itg, stg = c.h.solve_batch(*args)
    Qo, dQo, fo, ito, sto = c.o.solve_batch(*args, n_threads=c.nt)
    print(f"{sr.case_name(c.id)} ragged={ragged}: iterations gpu {itg.tolist()} oracle {ito.tolist()} status {stg.tolist()} "
          f"max |Q - Q_oracle| {np.abs(Qg - Qo).max():.3e}")
    np.testing.assert_array_equal(itg, ito)
    np.testing.assert_array_equal(stg, sto)
    assert np.isin(stg, OK).all() and (itg > 1).all()
    np.testing.assert_allclose(Qg, Qo, rtol=0, atol=1e-6)
    np.testing.assert_allclose(fg, fo, rtol=1e-8)
    # fresh handles: the launches for many instances in flight, the same without the step kernel's broad phase, and eight
    # waypoints asked of every obstacle workgroup -- bit for bit the same trajectories
    ref = None
    for env in ({"GTO_FEW_INSTANCES": "0"}, {"GTO_FEW_INSTANCES": "0", "GTO_PREBROAD": "0"}, {"GTO_OBS_TG": "8"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            h = c.handle(capi)
        got = h.solve_batch(*args)
        h.close()
        if ref is None:
            ref = got
            np.testing.assert_array_equal(ref[3], ito)
            np.testing.assert_array_equal(ref[4], sto)
            np.testing.assert_allclose(ref[0], Qo, rtol=0, atol=1e-6)
            np.testing.assert_allclose(ref[2], fo, rtol=1e-8)
        elif "GTO_FEW_INSTANCES" in env:
            for x, y in zip(ref, got):
                np.testing.assert_array_equal(x, y)
        else:
            for x, y in zip((Qg, dQg, fg, itg, stg), got):
                np.testing.assert_array_equal(x, y)
    return Qg


@pytest.mark.parametrize("cid", CASES, ids=sr.case_name)
def test_solve_matches_oracle(capi, rigs, monkeypatch, cid):
    c = rigs(cid)
    Q = _solve_against_oracle(capi, monkeypatch, c, ragged=False)
    d = c.desc
    assert np.abs(Q[:, :, 1] - Q[:, :, 0]).max() == 0.0 and np.array_equal(Q[:, :, 0], c.qc)
    assert (Q >= d.lower[None, :, None]).all() and (Q <= d.upper[None, :, None]).all()


@pytest.mark.parametrize("cid", [cid for cid in CASES if cid[0] in sr.RAGGED_KINDS], ids=sr.case_name)
def test_solve_of_ragged_goal_sets_matches_oracle(capi, rigs, monkeypatch, cid):
    c = rigs(cid)
    Q = _solve_against_oracle(capi, monkeypatch, c, ragged=True)
    a = c.h.eval_objective(0, c.goals_all, c.n_goals_ragged, c.S, c.base, Q)
    b = c.o.eval_objective(0, c.goals_all, c.n_goals_ragged, c.S, c.base, Q)
    np.testing.assert_array_equal(a[3], b[3])   # the goal the solved trajectory ends at


# ------------------------------------------------------------------------------------------------- IK
@pytest.mark.parametrize("cid", IK_CASES, ids=sr.case_name)
def test_ik_matches_oracle(rigs, cid):
    c = rigs(cid)
    for sid in (None, 0):
        qi, fi, iti, sti = c.h.solve_ik_batch(sid, c.qc, c.goals[:, 0], c.base, max_iter=sr.IK_MAX_ITER)
        qo, fo, ito, sto = c.o.solve_ik_batch(sid, c.qc, c.goals[:, 0], c.base, max_iter=sr.IK_MAX_ITER, n_threads=c.nt)
        np.testing.assert_array_equal(iti, ito)
        np.testing.assert_array_equal(sti, sto)
        assert np.isin(sti, OK).all()
        np.testing.assert_allclose(qi, qo, rtol=0, atol=1e-6)
        np.testing.assert_allclose(fi, fo, rtol=1e-8, atol=1e-12)
        q1, _, it1, st1 = c.h.solve_ik_batch(sid, c.qc, c.goals[:, 0], c.base, max_iter=0)
        assert (it1 == 0).all() and (st1 == 1).all() and q1.tobytes() == c.qc.tobytes()


@pytest.mark.parametrize("goal_kind", [pref.GTO_IK_GOAL_QUATERNION, pref.GTO_IK_GOAL_RPY])
@pytest.mark.parametrize("cid", IK_CASES, ids=sr.case_name)
def test_ik_to_pose_goals_matches_the_restatement(rigs, cid, goal_kind):
    """Without a scene, lock-step with tests/ik_pose_ref.py as tests/test_gpu_ik_pose_cases.py holds it: iterations and status
    equal, q to 1e-9, cost to rtol 1e-10.  With the scene: a regular end, not above the seed's cost, and the cost is the pose
    term plus the oracle's collision term at the returned q."""
    c = rigs(cid)
    goals = sr.pose_goals(c, goal_kind)
    q, f, it, st = c.h.solve_ik_pose_batch(goal_kind, None, c.qc, goals, None, max_iter=sr.POSE_MAX_ITER)
    qr, fr, itr, str_ = sr.pose_restatement(c, c.o, goal_kind)
    np.testing.assert_array_equal(it, itr)
    np.testing.assert_array_equal(st, str_)
    np.testing.assert_allclose(q, qr, rtol=0, atol=1e-9)
    np.testing.assert_allclose(f, fr, rtol=1e-10, atol=1e-15)
    qs, fs, its, sts = c.h.solve_ik_pose_batch(goal_kind, 0, c.qc, goals, c.base, max_iter=sr.POSE_MAX_ITER)
    f0 = c.h.solve_ik_pose_batch(goal_kind, 0, c.qc, goals, c.base, max_iter=0)[1]
    assert np.isfinite(qs).all() and np.isin(sts, OK).all() and (fs <= f0).all()
    Tq = c.o.eval_fk(qs)[:, c.desc.frame_index(c.ee)]
    val = np.stack([c.o.eval_points(0, qs[b:b + 1], c.base[b], use_obs=True)[2].sum() for b in range(c.B)])
    want = np.array([pref.pose_term(goal_kind, Tq[b], goals[b]) for b in range(c.B)]) + c.opts.w_obstacle * val
    np.testing.assert_allclose(fs, want, rtol=1e-9, atol=1e-13)


@pytest.mark.parametrize("cid", IK_CASES, ids=sr.case_name)
def test_ik_report_against_the_oracle(rigs, cid):
    """As tests/test_gpu_seed_waves.py::test_report_on_other_robots_against_the_oracle, at six instances."""
    import torch
    from test_gpu_grasp_chain import cu, dev_empty, widest_gap
    c = rigs(cid)
    d, h, o, B = c.desc, c.h, c.o, 6
    fe = d.frame_index(c.ee)
    rng = np.random.default_rng(31 + c.T)
    q = rng.uniform(d.lower, d.upper, (B, d.ndof))
    base = rng.uniform(-0.03, 0.03, (B, 3))
    off = rng.uniform(-1.0, 1.0, (B, d.ndof)) * np.linspace(0.0, 0.3, B)[:, None] * (d.upper - d.lower)[None, :]
    tf_o = o.eval_fk(q)[:, fe]
    RT = o.eval_fk(np.clip(q + off, d.lower, d.upper))[:, fe]
    cost_o = np.stack([o.eval_points(0, q[b:b + 1], base[b], use_obs=True)[2].sum(axis=1)[0] for b in range(B)])
    ep_o, er_o, _ = gref.report(tf_o, RT, cost_o, 1.0, 1.0, 1.0)
    assert ep_o[0] == 0 and er_o[0] < 1e-5
    pos_tol, m_pos = widest_gap(ep_o, 1e-3)
    rot_tol, m_rot = widest_gap(er_o, 1e-2)
    cost_tol, m_cost = widest_gap(cost_o, 1.0)
    assert m_pos > 1e-9 and m_rot > 1e-3 and m_cost > 1e-9 * max(1.0, np.abs(cost_o).max())
    acc = gref.report(tf_o, RT, cost_o, pos_tol, rot_tol, cost_tol)[2]
    outs = [dev_empty((B,), torch.float64) for _ in range(3)] + [dev_empty((B,), torch.uint8, 9)]
    keep = [cu(np.zeros(B, np.int32)), cu(q), cu(RT.reshape(B, 16)), cu(base)]
    torch.cuda.synchronize()
    h.ik_report_device(B, *[x.data_ptr() for x in keep], pos_tol, rot_tol, cost_tol, *[x.data_ptr() for x in outs])
    torch.cuda.synchronize()
    g_ep, g_er, g_cost, g_acc = [x.cpu().numpy() for x in outs]
    assert not np.isnan(g_er).any()
    np.testing.assert_allclose(g_ep, ep_o, rtol=0, atol=1e-12)
    np.testing.assert_allclose(g_er, er_o, rtol=0, atol=1e-5)
    np.testing.assert_allclose(g_cost, cost_o, rtol=1e-11, atol=0)
    assert np.array_equal(g_acc.astype(bool), acc)


@pytest.mark.parametrize("cid", IK_CASES, ids=sr.case_name)
def test_seed_choice_against_the_oracle(rigs, cid):
    """gto_seed_goalsets_device as tests/test_gpu_seed_waves.check_seeds holds it: every candidate's cost to 1e-12 and distance
    to 1e-14 of the oracle's, bit-equal to gto_plan_cost, the choice exact on the kernel's own scores and the oracle's where
    rounding cannot turn it, the seed built from it bit for bit.  There the limit is one instance left out of the comparison
    with the oracle's choice; here also those the case records as exact cost ties, whose choice rests on the distances alone."""
    from test_gpu_seed_waves import check_seeds, oracle_seeds
    c = rigs(cid)
    case = sr.seed_goalset_case(c)
    ties = sr.SEED_TIES.get(cid, 0)   # instances with an exact cost tie (tests/test_small_robots_cpu.py asserts the number)
    for f32 in (True, False):
        want = oracle_seeds(c, case, f32)
        assert sr.seed_cost_ties(want) == ties
        for interpolate in (True, False):
            left_out, worst = check_seeds(c, case, want, interpolate, f32)
            print(f"seeds {sr.case_name(cid)} interpolate={interpolate} f32={f32}: {left_out} of {c.B} left out of the oracle's "
                  f"choice ({ties} with tied costs), max rel seed_cost diff from the oracle {worst:.3e}")
            assert left_out <= 1 + ties


# ------------------------------------------------------------------------------------------------- base placement
def _base_placement(c, ragged):
    import torch
    goals, ng = (c.goals_all, c.n_goals_ragged) if ragged else (c.goals, c.n_goals)
    n_max = goals.shape[1]
    want = c.h.solve_base_batch(c.qc, goals, ng, 0.01, max_iter=sr.BASE_MAX_ITER)
    yo, qo, fo, ito, sto = c.o.solve_base_batch(c.qc, goals, ng, 0.01, max_iter=sr.BASE_MAX_ITER, n_threads=c.nt)
    yg, qg, fg, itg, stg = want
    np.testing.assert_array_equal(itg, ito)
    np.testing.assert_array_equal(stg, sto)
    assert np.isin(stg, OK).all()
    np.testing.assert_allclose(fg, fo, rtol=1e-7, atol=1e-12)
    np.testing.assert_allclose(yg, yo, rtol=0, atol=1e-6)
    live = ng[:, None] > np.arange(n_max)
    np.testing.assert_allclose(qg[live], qo[live], rtol=0, atol=1e-6)
    assert qg[~live].tobytes() == np.broadcast_to(c.qc[:, None], qg.shape)[~live].tobytes()   # rows past a set's goals: qc
    if c.kind in ("ee_above_joints", "static_links_only"):  # no joint moves the gripper's frame: every joint keeps qc's bits
        assert qg[live].tobytes() == np.broadcast_to(c.qc[:, None], qg.shape)[live].tobytes()
    # the device variant, bit for bit
    B, nd = c.B, c.desc.ndof
    d_y, d_q = torch.full((B, 3), -7.0, dtype=torch.float64, device="cuda"), torch.full((B, n_max, nd), -7.0, dtype=torch.float64, device="cuda")
    d_f, d_it, d_st = torch.empty(B, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    d_qc, d_goals = torch.from_numpy(np.ascontiguousarray(c.qc)).cuda(), torch.from_numpy(np.ascontiguousarray(goals)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    c.h.solve_base_batch_device(B, n_max, ng, d_qc.data_ptr(), d_goals.data_ptr(), 0.01, sr.BASE_MAX_ITER, d_y.data_ptr(), d_q.data_ptr(),
                                d_f.data_ptr(), d_it.data_ptr(), d_st.data_ptr(), s.cuda_stream)
    s.synchronize()
    for got, w in zip((d_y, d_q, d_f, d_it, d_st), want):
        assert got.cpu().numpy().tobytes() == w.tobytes()


@pytest.mark.parametrize("cid", IK_CASES, ids=sr.case_name)
def test_base_placement_matches_oracle(rigs, cid):
    _base_placement(rigs(cid), ragged=False)


@pytest.mark.parametrize("cid", [cid for cid in IK_CASES if cid[0] in sr.RAGGED_KINDS], ids=sr.case_name)
def test_base_placement_of_ragged_goal_sets_matches_oracle(rigs, cid):
    _base_placement(rigs(cid), ragged=True)


@pytest.mark.parametrize("cid", REPORT_CASES, ids=sr.case_name)
def test_base_report_against_the_restatement(rigs, cid):
    from test_gpu_base_chain import ERR_POS_TOL, ERR_ROT_TOL, occupancy, run_report, same_grid
    c = rigs(cid)
    d, B, n_max = c.desc, sr.REPORT_B, sr.REPORT_N_MAX
    case = sr.base_report_case(c, c.o)
    occ = occupancy(case.cloud, epsilon=case.epsilon)
    same_grid(occ, case.grid)
    ep, er, col, ff = run_report(c.h, occ, case, B, n_max)
    w_ep, w_er = bref.report(c.o, d.frame_index(c.ee), d.frame_index(c.gripper), case.goals, case.n_goals, case.y, case.q, fill=-7.0)
    w_col = bref.collisions(case.grid, case.foot, case.y, case.qc)
    live = case.n_goals[:, None] > np.arange(n_max)
    assert (ep[~live] == -7.0).all() and (er[~live] == -7.0).all()
    np.testing.assert_allclose(ep[live], w_ep[live], rtol=0, atol=ERR_POS_TOL)
    np.testing.assert_allclose(er[live], w_er[live], rtol=0, atol=ERR_ROT_TOL)
    np.testing.assert_array_equal(col, w_col)
    assert (w_col == 0).any() and (w_col > 0).any() and ff[0] == bref.first_free(w_col)
    occ.close()


# ------------------------------------------------------------------------------------------------- check_plans
@pytest.mark.parametrize("cid", PLAN_CASES, ids=sr.case_name)
def test_check_plans_on_a_depth_observation_equals_oracle(rigs, monkeypatch, cid):
    from grasptrajopt_amd.observation import Observation
    c = rigs(cid)
    inst, world_points = sr.plan_depth_instance(c, c.o)
    obs = Observation.from_depth(inst.depth, inst.K, inst.cam, None, inst.threshold)
    poisoned = inst.plans.copy()
    poisoned[inst.nan_at] = np.nan
    p, _, t = inst.nan_at
    for bases in (inst.base, inst.bases):
        want, n_undecided = dc.plan_expected(inst, c.desc, world_points, bases)
        assert n_undecided == 0 and (want == 0).any() and want[p, t] == -1
        assert (want > 0).any() == (c.kind != "static_links_only")   # (nothing moves there: the second half hides behind the image too)
        np.testing.assert_array_equal(c.h.check_plans(obs, poisoned, bases), want)
        clean = c.h.check_plans(obs, inst.plans, bases)
        assert clean[p, t] >= 0
        clean[p, t] = -1
        np.testing.assert_array_equal(clean, want)
        for tg in ("1", "3"):
            monkeypatch.setenv("GTO_CHECK_TG", tg)
            np.testing.assert_array_equal(c.h.check_plans(obs, poisoned, bases), want, err_msg=f"GTO_CHECK_TG={tg}")
        monkeypatch.delenv("GTO_CHECK_TG")
    obs.close()


@pytest.mark.parametrize("cid", PLAN_CASES, ids=sr.case_name)
def test_check_plans_on_a_cloud_observation_equals_oracle(rigs, monkeypatch, cid):
    import torch
    from grasptrajopt_amd.observation import Observation
    c = rigs(cid)
    inst, world_points = sr.plan_cloud_instance(c, c.o)
    obs = Observation.from_cloud(inst.points, inst.normals, cc.PLAN_K)
    poisoned = inst.plans.copy()
    poisoned[inst.nan_at] = np.nan
    p, _, t = inst.nan_at
    want = {}
    for variant, bases in (("shared", inst.base), ("per_plan", inst.bases)):
        counts, n_undecided = cc.plan_expected(inst, c.desc, world_points, bases)
        want[variant] = counts
        assert n_undecided == 0 and counts[p, t] == -1
        np.testing.assert_array_equal(c.h.check_plans(obs, poisoned, bases), counts, err_msg=variant)
        with exhaustive():
            np.testing.assert_array_equal(c.h.check_plans(obs, poisoned, bases), counts, err_msg=f"{variant}, exhaustive")
    bad_bases = inst.bases.copy()
    bad_bases[2, 1] = np.nan
    expect = want["per_plan"].copy()
    expect[2] = -1
    np.testing.assert_array_equal(c.h.check_plans(obs, poisoned, bad_bases), expect)
    for tg in ("1", "2", "3", "4"):
        monkeypatch.setenv("GTO_CHECK_TG", tg)
        np.testing.assert_array_equal(c.h.check_plans(obs, poisoned, inst.bases), want["per_plan"], err_msg=f"GTO_CHECK_TG={tg}")
    monkeypatch.delenv("GTO_CHECK_TG")
    side = torch.cuda.Stream(device="cuda:0")
    d_plans = torch.as_tensor(poisoned, dtype=torch.float64).to("cuda:0")
    d_count = torch.full((dc.PLAN_B, c.T), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    c.h.check_plans_device(obs, dc.PLAN_B, d_plans.data_ptr(), d_count.data_ptr(), inst.base, stream=side.cuda_stream)
    side.synchronize()
    np.testing.assert_array_equal(d_count.cpu().numpy(), want["shared"])
    obs.close()


# ------------------------------------------------------------------------------------------------- retiming
@pytest.mark.parametrize("subdiv", sr.RETIME_SUBDIVS)
@pytest.mark.parametrize("T", [4, 5])
@pytest.mark.parametrize("kind", sr.RETIME_KINDS)
def test_retime_against_the_restatement(rigs, kind, T, subdiv):
    """tests/test_gpu_retime._check_against_ref on plans of one and two joints over 4 and 5 waypoints; plan 1 has joint 0
    standing still (with one joint: no moving joint, duration 0); repeats, a plan on its own and the reversed batch give the
    same bits."""
    from test_gpu_retime import KEYS, _check_against_ref, _derived_checks, _same
    c = rigs((kind, T, (5, 5, 5)))
    d, plans, vm, am = sr.retime_inputs(kind, T)
    assert d.ndof == c.desc.ndof and c.h.T == T
    g = _check_against_ref(d, c.h, plans, subdiv=subdiv, M=16, vmax=vm, amax=am)
    assert (g["status"] == 0).all() and g["t_grid"].shape == (sr.RETIME_B, subdiv * (T - 1) + 1)
    if d.ndof == 1:  # the stationary plan, as tests/test_gpu_retime.py::test_stationary_plan states it
        assert g["duration"][1] == 0 and np.all(g["t_grid"][1] == 0) and np.all(g["sd_grid"][1] == 0)
        assert np.all(g["q"][1] == plans[1][:, 0]) and np.all(g["qd"][1] == 0) and np.all(g["qdd"][1] == 0)
    moving = np.flatnonzero(g["duration"] > 0)
    assert len(moving) == sr.RETIME_B - (d.ndof == 1)
    _derived_checks(d, plans[moving], {k: v[moving] for k, v in g.items()}, vm, am, subdiv=subdiv)
    again = c.h.retime_batch(plans, vm, am, subdiv=subdiv, n_samples=16)
    rev = c.h.retime_batch(plans[::-1].copy(), vm, am, subdiv=subdiv, n_samples=16)
    for k in KEYS + ("status",):
        assert _same(again[k], g[k]) and _same(rev[k][::-1], g[k]), k
    for i in range(sr.RETIME_B):
        one = c.h.retime_batch(plans[i:i + 1], vm, am, subdiv=subdiv, n_samples=16)
        for k in KEYS:
            assert _same(one[k][0], g[k][i]), (k, i)


@pytest.mark.parametrize("subdiv", sr.RETIME_SUBDIVS)
@pytest.mark.parametrize("T", [4, 5])
@pytest.mark.parametrize("kind", sr.RETIME_KINDS)
def test_retime_convex_against_the_restatement(rigs, kind, T, subdiv):
    """gto_retime_paths_convex on the same plans: tests/test_gpu_retime_convex._against_reference_and_greedy (the restatement's
    statuses and durations within the certified gap, feasibility and samples recomputed from the outputs, never longer than
    the greedy profile, the greedy outputs untouched) at one and two joints and N = 4 gridpoints (two variables) upwards;
    with one joint plan 1 has no moving joint: duration 0 and no Newton step."""
    import retime_convex_ref as cr
    from test_gpu_retime_convex import GAP_TOL, _against_reference_and_greedy
    c = rigs((kind, T, (5, 5, 5)))
    d, plans, vm, am = sr.retime_inputs(kind, T)
    assert d.ndof == c.desc.ndof and subdiv * (T - 1) + 1 >= 4
    with np.errstate(divide="ignore", invalid="ignore"):
        r = cr.retime_paths_convex_ref(plans, None, vm, am, subdiv, 16, GAP_TOL)
    g = _against_reference_and_greedy(c.h, plans, None, vm, am, subdiv, r, M=16)
    assert (g["status"] == 0).all() and g["t_grid"].shape == (sr.RETIME_B, subdiv * (T - 1) + 1)
    still = d.ndof == 1
    assert (g["duration"] > 0).sum() == sr.RETIME_B - still and (g["iters"] > 0).sum() == sr.RETIME_B - still
    assert not still or (g["duration"][1] == 0 and g["iters"][1] == 0)


@pytest.mark.parametrize("subdiv", sr.RETIME_SUBDIVS)
@pytest.mark.parametrize("T", [4, 5])
@pytest.mark.parametrize("kind", sr.RETIME_KINDS)
def test_retime_torque_against_the_restatement(capi, kind, T, subdiv):
    """gto_retime_paths_torque on the same plans and limits with seeded link inertials, the `full` payload and tau_max at 1.5 to
    3 times the unloaded robot's largest static torque (sr.retime_torque_inputs): tests/test_gpu_retime_torque._against_reference
    (the restatement's statuses and durations within the certified gap, limits and torques recomputed from the outputs,
    tau_out bit for bit gto_inverse_dynamics of the samples).  With one joint plan 1 stands still: duration 0, no Newton step
    and tau the static torque at every sample where the joint can hold the payload, INFEASIBLE and NaN where it cannot
    (sr.RETIME_STILL_HELD, asserted on the CPU).  Without any finite limit the call is the convex call, bit for bit."""
    import dynamics_ref as dr
    import retime_torque_ref as tr
    from test_gpu_retime import KEYS, _same
    from test_gpu_retime_torque import GAP_TOL, INFEASIBLE, _against_reference
    d, fee, plans, vm, am, tm, pl = sr.retime_torque_inputs(kind, T, subdiv)
    r0 = sr.Robot(kind, seed=sr.SEEDS.get((kind, T, (5, 5, 5)), 0))
    h = capi.SolverHandle(d, r0.ee, r0.gripper, device=0, n_gripper_points=r0.n_gripper_points)
    try:
        with np.errstate(divide="ignore", invalid="ignore"):
            r = tr.retime_paths_torque_ref(d, fee, plans, None, vm, am, tm, pl, subdiv, 16, GAP_TOL)
        g, convex = _against_reference(d, fee, h, plans, None, vm, am, tm, pl, subdiv, r, M=16)
        assert np.isfinite(tm).all() and np.isin(g["status"], (0, INFEASIBLE)).all() and (g["status"] == 0).sum() >= 2
        if d.ndof == 1:
            held = sr.RETIME_STILL_HELD[kind, T]
            assert g["status"][1] == (0 if held else INFEASIBLE) and g["iters"][1] == 0
            if held:
                static = dr.inverse_dynamics(d, plans[1][:, 0], np.zeros(1), np.zeros(1), fee, tr.payload_of(pl, 1))
                want = h.inverse_dynamics(plans[1][:, 0], np.zeros(1), np.zeros(1), {k: v[1:2] for k, v in zip(("mass", "com", "inertia"), pl)})
                assert g["duration"][1] == 0 and _same(g["tau"][1], np.tile(want, (16, 1)))
                assert np.abs(g["tau"][1] - static).max() <= 1e-11 * max(1.0, np.abs(static).max())
            else:
                assert np.isnan(g["duration"][1]) and np.isnan(g["tau"][1]).all()
        free = h.retime_paths_torque(plans, vm, am, tau_max=np.inf, payload={k: v for k, v in zip(("mass", "com", "inertia"), pl)},
                                     subdiv=subdiv, n_samples=16, gap_tol=GAP_TOL)
        for k in KEYS + ("status", "iters"):  # no row is added: the convex call's arithmetic
            assert _same(free[k], convex[k]), k
    finally:
        h.close()
