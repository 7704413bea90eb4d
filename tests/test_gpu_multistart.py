"""GPU: several seeds per goal set and the best of their plans -- gto_seed_goalsets_multi_device, gto_plan_report_device,
gto_select_plans_device and GraspChain.plan_objects(n_seeds=k) -- against gto_seed_goalsets_device, gto_eval_objective,
gto_ik_report_device, gto_solve_batch of a single seed and the numpy restatement (tests/multistart_ref.py).  Run the file
under a time limit (timeout -k 10 900 pytest ...) and stop at the first fault."""
import numpy as np
import pytest

import grasp_chain_ref as ref
import grasptrajopt_amd as g
import multistart_ref as mref
from grasptrajopt_amd import synthetic as syn
from seed_cases import WIDE_B, seed_case_wide, wide_rows
from test_gpu_grasp_chain import (IK_ITERS, chain_setup, cu, dev_empty, handle_with_scenes, run_seeds, same_bits, seed_case,
                                  widest_gap)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as gr
    gr.build()
    from grasptrajopt_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def panda(capi, oracle_mod):
    prob, h, _ = handle_with_scenes(capi, oracle_mod, "panda", 8, scene_seeds=(5, 9))
    yield prob, h
    h.close()


# ------------------------------------------------------------------------------------------------- 1. seeds
def run_seeds_multi(h, T, K, qc, qs, goals, n_goals, accept, sid, base, interpolate, f32):
    import torch
    B, n_max, ndof = qs.shape
    keep = [cu(sid), cu(qc), cu(goals), cu(n_goals), cu(qs), None if accept is None else cu(accept), cu(base)]
    outs = dict(goals_out=dev_empty((B, K, n_max, 16), torch.float64, -7.0), n_goals_out=dev_empty((B, K), torch.int32, -7),
                n_accepted=dev_empty((B,), torch.int32, -7), rows=dev_empty((B, n_max), torch.int32, -7),
                Q0=dev_empty((B, K, ndof, T), torch.float64, -7.0), seed_index=dev_empty((B, K), torch.int32, -7),
                seed_cost=dev_empty((B, n_max), torch.float64, -7.0), seed_dist=dev_empty((B, n_max), torch.float64, -7.0))
    torch.cuda.synchronize()
    h.seed_goalsets_multi_device(B, n_max, K, *[None if x is None else x.data_ptr() for x in keep], interpolate, f32,
                                 *[x.data_ptr() for x in outs.values()])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


def check_slots(got, plain, b, r, K, T):
    """Instance b of a K-slot call against the restatement r (mref.seed_slots) and the plain entry point's scores."""
    na, cnt = r["n_accepted"], r["n_goals_out"]
    assert got["n_accepted"][b] == na and (got["n_goals_out"][b] == cnt).all(), b
    for s in range(K):
        assert got["goals_out"][b, s, :cnt].tobytes() == r["goals_out"].tobytes(), (b, s)
        assert (got["goals_out"][b, s, cnt:] == -7.0).all(), (b, s)  # untouched
    assert got["rows"][b, :na].tolist() == r["rows"][:na].tolist() and (got["rows"][b, na:] == -7).all(), b
    for key in ("seed_cost", "seed_dist"):
        assert got[key][b].tobytes() == plain[key][b].tobytes(), (b, key)
    assert got["seed_index"][b].tolist() == r["seed_index"].tolist(), (b, got["seed_index"][b], r["seed_index"])
    if na:  # on the kernel's own scores
        order = np.lexsort((got["seed_dist"][b, :na], got["seed_cost"][b, :na]))[:K]
        assert got["seed_index"][b, :len(order)].tolist() == order.tolist(), b
    assert got["Q0"][b].tobytes() == r["Q0"].tobytes() or same_bits(got["Q0"][b], r["Q0"]), b  # (a NaN solution: a NaN on both sides)


@pytest.mark.parametrize("interpolate", [True, False])
def test_one_seed_is_the_plain_entry_point_in_every_output(panda, interpolate):
    import torch
    prob, h = panda
    case = seed_case(prob, np.random.default_rng(11), 8, 6)
    plain = run_seeds(h, torch, h.T, *case, interpolate, True)
    got = run_seeds_multi(h, h.T, 1, *case, interpolate, True)
    for key, v in plain.items():
        assert got[key].reshape(v.shape).tobytes() == v.tobytes(), key
    for b in range(8):
        assert got["rows"][b].tolist() == ref.accepted_rows(case[3][b], 6, case[4][b]).tolist() + [-7] * (6 - plain["n_accepted"][b]), b


@pytest.mark.parametrize("interpolate", [True, False])
def test_three_seeds_on_0_1_2_3_and_5_accepted_rows_are_the_restatement(panda, interpolate):
    import torch
    prob, h = panda
    d, T, K, n_max = prob.desc, h.T, 3, 6
    counts = [0, 1, 2, 3, 5, 6]
    rng = np.random.default_rng(12)
    qc, qs, goals, n_goals, accept, sid, base = [x[:len(counts)].copy() for x in seed_case(prob, rng, 8, n_max)]
    n_goals[:] = n_max
    for b, c in enumerate(counts):
        accept[b] = 0
        accept[b, rng.permutation(n_max)[:c]] = 1
    qs[5, 4] = qs[5, 1]  # a tie in cost and distance: the lower position first
    case = (qc, qs, goals, n_goals, accept, sid, base)
    plain = run_seeds(h, torch, T, *case, interpolate, True)
    got = run_seeds_multi(h, T, K, *case, interpolate, True)
    for b, c in enumerate(counts):
        r = mref.seed_slots(qc[b], goals[b], n_goals[b], qs[b], accept[b], T, h.opts.standoff_offset, d.param_index, interpolate, True,
                            lambda plans, b=b: h.plan_cost(int(sid[b]), plans, base[b])[0], K)
        assert r["n_accepted"] == c and (r["seed_index"] >= 0).sum() == min(c, K)
        check_slots(got, plain, b, r, K, T)
    assert got["seed_cost"][5, 1].tobytes() == got["seed_cost"][5, 4].tobytes() and got["seed_dist"][5, 1].tobytes() == got["seed_dist"][5, 4].tobytes()
    # any position in any batch: reversed, and one instance on its own
    rev = run_seeds_multi(h, T, K, *[x[::-1].copy() for x in case], interpolate, True)
    one = run_seeds_multi(h, T, K, *[x[4:5].copy() for x in case], interpolate, True)
    for key in got:
        assert rev[key][::-1].tobytes() == got[key].tobytes(), key
        assert one[key].tobytes() == got[key][4:5].tobytes(), key
    # a slot's seed is what the plain entry point chooses when only that slot's row is accepted
    b = 4
    rows = ref.accepted_rows(n_goals[b], n_max, accept[b])
    for s in range(K):
        only = np.zeros((1, n_max), np.uint8)
        only[0, rows[got["seed_index"][b, s]]] = 1
        alone = run_seeds(h, torch, T, qc[b:b + 1], qs[b:b + 1], goals[b:b + 1], n_goals[b:b + 1], only, sid[b:b + 1], base[b:b + 1], interpolate, True)
        assert alone["Q0"][0].tobytes() == got["Q0"][b, s].tobytes(), s


@pytest.mark.parametrize("n_max,K", [(65, 3), (130, 3), (130, 16)])
def test_ranked_seeds_on_goal_sets_wider_than_a_wave(panda, n_max, K):
    """The twelve instances of seed_cases.seed_case_wide (accepted rows, bit-equal ties and NaN solutions across the chunks of
    64 rows); instances 2 and 11 name no scene, so every cost of theirs is NaN and the distance decides."""
    import torch
    prob, h = panda
    d, T = prob.desc, h.T
    case = list(seed_case_wide(d, prob.qc[0], np.random.default_rng(100 + n_max), n_max))
    case[5] = case[5].copy()
    case[5][[2, 11]] = (-1, 7)
    qc, qs, goals, n_goals, accept, sid, base = case
    plain = run_seeds(h, torch, T, *case, True, False)
    got = run_seeds_multi(h, T, K, *case, True, False)
    for b in range(WIDE_B):
        na = int(plain["n_accepted"][b])
        r = mref.seed_slots(qc[b], goals[b], n_goals[b], qs[b], accept[b], T, h.opts.standoff_offset, d.param_index, True, False,
                            lambda plans, b=b, na=na: plain["seed_cost"][b, :na], K)
        # (the restatement forms the distances itself; a NaN distance is a NaN on both sides)
        assert np.array_equal(np.isnan(r["seed_dist"]), np.isnan(plain["seed_dist"][b, :na])), b
        fin = ~np.isnan(r["seed_dist"])
        assert r["seed_dist"][fin].tobytes() == plain["seed_dist"][b, :na][fin].tobytes(), b
        check_slots(got, plain, b, r, K, T)
    assert np.isnan(got["seed_cost"][2, :plain["n_accepted"][2]]).all() and (got["seed_index"][2] >= 0).sum() == min(K, plain["n_accepted"][2])
    assert np.isnan(got["seed_cost"][11, :plain["n_accepted"][11]]).all() and (got["seed_index"][11] >= 0).sum() == min(K, plain["n_accepted"][11])
    assert (got["seed_index"][1] == -1).all() and got["n_accepted"][1] == 0
    R = wide_rows(n_max)  # instance 6: every row accepted, copies of one solution across chunks: ranked by position
    for rows in (R["ties3"], R["ties2"]):
        ranks = [got["seed_index"][6].tolist().index(p) for p in rows if p in got["seed_index"][6]]
        assert ranks == sorted(ranks)
    rev = run_seeds_multi(h, T, K, *[x[::-1].copy() for x in case], True, False)
    for key in got:
        assert rev[key][::-1].tobytes() == got[key].tobytes(), key


# ------------------------------------------------------------------------------------------------- 2. report
def run_report(h, goals, n_goals, S, Q):
    import torch
    B, n_max = goals.shape[:2]
    keep = [cu(goals), cu(n_goals), None if S is None else cu(np.tile(np.asarray(S, dtype=np.float64).reshape(1, 16), (B, 1))), cu(Q)]
    outs = dict(goal_index=dev_empty((B,), torch.int32, -7), goal_cost=dev_empty((B,), torch.float64, -7.0),
                err_pos=dev_empty((B,), torch.float64, -7.0), err_rot=dev_empty((B,), torch.float64, -7.0))
    torch.cuda.synchronize()
    h.plan_report_device(B, n_max, *[None if x is None else x.data_ptr() for x in keep], *[x.data_ptr() for x in outs.values()])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


@pytest.mark.parametrize("standoff", [True, False])
def test_plan_report_against_eval_objective_and_ik_report(panda, standoff):
    import torch
    prob, h = panda
    d, T, B, n_max = prob.desc, h.T, 6, 4
    rng = np.random.default_rng(41)
    fe = d.frame_index(prob.cfg["link_ee"])
    # plans that end near their first goal configuration; goals: the frames of link_ee at configurations around it
    Q = np.stack([syn.make_seed(prob.qc[b], prob.qgoal[b, 0], T, d.param_index) for b in range(B)])
    Q[:, d.opt_index, 2:] += rng.uniform(-0.02, 0.02, (B, d.n_opt, T - 2))
    qg = np.tile(Q[:, None, :, T - 1], (1, n_max, 1))
    qg[:, :, d.opt_index] += rng.uniform(-0.15, 0.15, (B, n_max, d.n_opt))
    qg = np.clip(qg, d.lower, d.upper)
    goals = h.eval_fk(qg.reshape(-1, d.ndof))[:, fe].reshape(B, n_max, 16)
    n_goals = np.array([1, n_max, 3, n_max, 2, 1], np.int32)
    S = syn.standoff_pose(-0.1, prob.cfg["axis_standoff"]) if standoff else None
    base = np.zeros((B, 3))
    f_goal, _, _, argmin = h.eval_objective(0, goals, n_goals, S, base, Q)
    # every goal's term on its own: the two lowest of a set differ by more than 1e-9 relative
    terms = np.stack([h.eval_objective(0, goals[:, j:j + 1], 1, S, base, Q)[0] for j in range(n_max)], axis=1)
    for b in range(B):
        t = np.sort(terms[b, :n_goals[b]])
        assert len(t) == 1 or t[1] - t[0] > 1e-9 * t[1], (b, t)
        assert argmin[b] == int(np.argmin(terms[b, :n_goals[b]]))
    assert (argmin > 0).any()  # not every set ends at goal 0
    got = run_report(h, goals, n_goals, S, Q)
    assert got["goal_index"].tolist() == argmin.tolist()
    print("plan report standoff", standoff, "max rel |goal_cost - f_goal|", (np.abs(got["goal_cost"] - f_goal) / np.abs(f_goal)).max())
    np.testing.assert_allclose(got["goal_cost"], f_goal, rtol=1e-12, atol=0)
    # the errors: gto_ik_report_device of the last columns against the chosen goals, bit for bit
    outs = [dev_empty((B,), torch.float64) for _ in range(2)]
    keep = [cu(Q[:, :, T - 1]), cu(goals[np.arange(B), argmin])]
    torch.cuda.synchronize()
    h.ik_report_device(B, None, keep[0].data_ptr(), keep[1].data_ptr(), None, 0.01, 5.0, 5.0, outs[0].data_ptr(), outs[1].data_ptr())
    torch.cuda.synchronize()
    assert got["err_pos"].tobytes() == outs[0].cpu().numpy().tobytes() and got["err_rot"].tobytes() == outs[1].cpu().numpy().tobytes()
    assert (got["err_pos"] > 0).all() and np.isfinite(got["err_pos"]).all() and np.isfinite(got["err_rot"]).all()
    # a plan with a NaN: -1 and NaNs, and nobody else's result changes; one plan on its own
    Q2 = Q.copy()
    Q2[2, d.opt_index[1], 17] = np.nan
    bad = run_report(h, goals, n_goals, S, Q2)
    assert bad["goal_index"][2] == -1 and all(np.isnan(bad[k][2]) for k in ("goal_cost", "err_pos", "err_rot"))
    for k in got:
        assert np.delete(bad[k], 2).tobytes() == np.delete(got[k], 2).tobytes(), k
    one = run_report(h, goals[3:4], n_goals[3:4], S, Q[3:4])
    for k in got:
        assert one[k].tobytes() == got[k][3:4].tobytes(), k
    h.plan_report_device(0, 1, None, None, None, None)  # B = 0: no launch, no argument looked at


# ------------------------------------------------------------------------------------------------- 3. select
def run_select(h, B, K, status, cost, ep, er, counts, Q, dQ, pos_tol=0.01, rot_tol=5.0, max_points=5):
    import torch
    keep = [cu(status), cu(cost), cu(ep), cu(er), None if counts is None else cu(counts)]
    dQ_, dD_ = cu(Q), cu(dQ)
    outs = dict(best=dev_empty((B,), torch.int32, -7), cls=dev_empty((B,), torch.int32, -7),
                Q=dev_empty((B,) + Q.shape[2:], torch.float64, -7.0), dQ=dev_empty((B,) + dQ.shape[2:], torch.float64, -7.0))
    torch.cuda.synchronize()
    h.select_plans_device(B, K, *[None if x is None else x.data_ptr() for x in keep], pos_tol, rot_tol, max_points, dQ_.data_ptr(),
                          dD_.data_ptr(), *[x.data_ptr() for x in outs.values()])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


@pytest.mark.parametrize("K", [1, 2, 16])
@pytest.mark.parametrize("B", [1, 3])
def test_select_on_crafted_slots(panda, B, K):
    prob, h = panda
    T, ndof, NT = h.T, prob.desc.ndof, len(mref.CLASS_TABLE)
    rng = np.random.default_rng(100 * B + K)
    seen = set()
    for trial in range(6):
        if K == 16 and trial == 0:
            rows = np.stack([np.concatenate([np.roll(np.arange(NT), -3 * b), rng.integers(0, NT, K - NT)]) for b in range(B)])
        elif K == 2 and trial == 0:
            rows = np.stack([[9, 0], [7, 8], [4, 3]][:B])  # a tie on (class, cost); a NaN cost behind inf; the lower cost of a class
        else:
            rows = rng.integers(0, NT, (B, K))
        (status, cost, ep, er, c3), cls = mref.class_table(rows.reshape(-1))
        counts = np.zeros((B * K, T), np.int32)
        counts[np.arange(B * K)[:, None], rng.permutation(T)[:3][None, :]] = c3  # the three counts anywhere among the waypoints
        shape = lambda x: x.reshape((B, K) + x.shape[1:])
        status, cost, ep, er, counts = map(shape, (status, cost, ep, er, counts))
        Q, dQ = rng.standard_normal((B, K, ndof, T)), rng.standard_normal((B, K, ndof, T - 1))
        for use_counts in (True, False):
            got = run_select(h, B, K, status, cost, ep, er, counts if use_counts else None, Q, dQ)
            for b in range(B):
                best, c, all_cls = mref.select(status[b], cost[b], ep[b], er[b], counts[b] if use_counts else None, 0.01, 5.0, 5)
                assert (got["best"][b], got["cls"][b]) == (best, c), (b, rows[b], use_counts)
                assert got["Q"][b].tobytes() == Q[b, best].tobytes() and got["dQ"][b].tobytes() == dQ[b, best].tobytes(), b
                if use_counts:
                    assert all_cls == [cls[b * K + s] for s in range(K)]
                    seen.update(all_cls)
        # every slot on its own (n_seeds = 1 over B K objects): its class, and its own rows back
        flat = run_select(h, B * K, 1, *[x.reshape((B * K, 1) + x.shape[2:]) for x in (status, cost, ep, er, counts, Q, dQ)])
        assert flat["cls"].tolist() == cls and (flat["best"] == 0).all() and flat["Q"].tobytes() == Q.tobytes()
    assert K < 16 or seen == {0, 1, 2, 3, 4}
    with pytest.raises(g._capi.GTOError, match=r"\(-4\).*n_seeds"):
        h.select_plans_device(1, 17, 1, 1, 1, 1, None, 0.01, 5.0, 5)
    with pytest.raises(g._capi.GTOError, match=r"\(-4\).*n_seeds"):
        h.seed_goalsets_multi_device(1, 1, 0, 1, 1, 1, 1, 1, None, 1, 1, 1)
    with pytest.raises(g._capi.GTOError, match=r"\(-4\).*65535"):
        h.seed_goalsets_multi_device(4096, 1, 16, 1, 1, 1, 1, 1, None, 1, 1, 1)
    h.select_plans_device(0, 3, None, None, None, None, None, 0.01, 5.0, 5)  # B = 0: no launch


def test_entry_points_validate_on_the_host(panda, capi):
    import torch
    from helpers import limit_robot
    _, h = panda
    x = dev_empty((64,), torch.float64, 0.0).data_ptr()
    h.seed_goalsets_multi_device(0, 1, 3, None, None, None, None, None, None, None, 1, 1)  # B = 0: no launch, no argument looked at
    for call in (lambda: h.seed_goalsets_multi_device(1, 0, 3, x, x, x, x, x, None, x, 1, 1),      # n_max < 1
                 lambda: h.seed_goalsets_multi_device(1, 1, 3, x, x, x, x, None, None, x, 1, 1),   # no q_solutions
                 lambda: h.plan_report_device(1, 1, x, x, None, None),                             # no plans
                 lambda: h.plan_report_device(1, 0, x, x, None, x),
                 lambda: h.select_plans_device(1, 2, x, x, x, None, None, 0.01, 5.0, 5),           # no err_rot
                 lambda: h.select_plans_device(1, 2, x, x, x, x, None, 0.01, 5.0, 5, Q_out=x)):    # a copy asked for without its source
        with pytest.raises(capi.GTOError, match=r"\(-1\)"):
            call()
    desc, ee = limit_robot("chain", n_opt=9)
    hw = capi.SolverHandle(desc, ee, ee, device=0)
    for call in (lambda: hw.seed_goalsets_multi_device(1, 1, 3, x, x, x, x, x, None, x, 1, 1),
                 lambda: hw.plan_report_device(1, 1, x, x, None, x),
                 lambda: hw.select_plans_device(1, 2, x, x, x, x, None, 0.01, 5.0, 5)):
        with pytest.raises(capi.GTOError, match=r"\(-4\).*eight optimised joints"):
            call()
    hw.close()


# ------------------------------------------------------------------------------------------------- 4. the chain
CHAIN_FIELDS = ("plans", "dQ", "cost", "iters", "status", "n_accepted", "seed_index", "seed_cost", "seed_dist", "q_solutions", "err_pos",
                "err_rot", "ik_cost", "ik_iters", "ik_status", "accept", "counts")
MULTI_FIELDS = CHAIN_FIELDS + ("best_slot", "plan_class", "goal_index", "goal_row", "plan_err_pos", "plan_err_rot", "slot_cost",
                               "slot_class", "slot_plans")
PER_GRASP = ("q_solutions", "err_pos", "err_rot", "ik_cost", "ik_iters", "ik_status", "accept")  # rows behind n_grasps are padding


@pytest.fixture(scope="module")
def eight():
    """Eight objects of up to five grasps over two scenes, as in test_chain_of_eight_objects_over_two_scenes_is_eight_single_calls:
    IK stopped early and a position threshold in the widest gap of the host's own report, so that some grasps pass."""
    from grasptrajopt_amd.grasp_chain import GraspChain
    B, n = 8, 5
    cfg, robot, fields, RT = chain_setup("panda", B * n, seed=33)
    RT = RT.reshape(B, n, 4, 4)
    rng = np.random.default_rng(2)
    qc = np.tile(np.array(cfg["default_pose"], dtype=np.float64), (B, 1))
    qc[:, robot.desc.opt_index] += rng.uniform(-0.1, 0.1, (B, robot.desc.n_opt))
    base = rng.uniform(-0.02, 0.02, (B, 3))
    n_grasps = np.array([5, 3, 5, 1, 4, 5, 2, 5], np.int32)
    per_obj = [fields[b % 2] for b in range(B)]
    ik = g.IKSolver(robot, cfg["link_ee"], cfg["link_gripper"], collision_avoidance=True)
    ik.max_iter = IK_ITERS
    host = [ik.solve_ik_batch(qc[b], RT[b], per_obj[b][1], base[b]) for b in range(B)]
    ep, cost = (np.stack([h_[i] for h_ in host]) for i in (1, 3))
    counted = np.arange(n)[None, :] < n_grasps[:, None]
    pos_tol, margin = widest_gap(ep[counted], 1e-3)
    assert margin > 1e-9
    chain = GraspChain(robot, cfg["link_ee"], cfg["link_gripper"])
    chain.max_iter, chain.ik_max_iter = 30, IK_ITERS
    obs = g.DepthPointCloud(*syn.wall_scene()[:3], target_mask=syn.wall_scene()[3], threshold=1.5).observation()
    kw = dict(axis_standoff=cfg["axis_standoff"], pos_tol=pos_tol, rot_tol_deg=360.0, ik_collision_threshold=float(np.abs(cost).max()) * 2.0 + 1.0,
              observation=obs)
    args = (qc, RT, RT, n_grasps, per_obj, base)
    three = chain.plan_objects(*args, n_seeds=3, **kw)
    yield dict(cfg=cfg, robot=robot, chain=chain, args=args, kw=kw, three=three, B=B, n=n)
    chain.close()
    robot.close()


def test_chain_with_one_seed_is_the_chain_without_the_argument(eight):
    chain, args, kw = eight["chain"], eight["args"], eight["kw"]
    a, b = chain.plan_objects(*args, **kw), chain.plan_objects(*args, n_seeds=1, **kw)
    assert sorted(vars(a)) == sorted(vars(b)) == sorted(CHAIN_FIELDS)
    for k in CHAIN_FIELDS:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes() and getattr(a, k).dtype == getattr(b, k).dtype, k
    assert a.seed_index.shape == (eight["B"],)
    with pytest.raises(ValueError):
        chain.plan_objects(*args, n_seeds=17, **kw)


def test_chain_with_three_seeds_solves_every_seed_and_keeps_the_best(eight):
    chain, (qc, RT, _, n_grasps, _, base), kw, r = eight["chain"], eight["args"], eight["kw"], eight["three"]
    B, n, K, cfg = eight["B"], eight["n"], 3, eight["cfg"]
    h, d, T = chain._handle, chain.robot.desc, chain.T
    S = syn.standoff_pose(chain.standoff_distance, cfg["axis_standoff"])
    one = chain.plan_objects(*eight["args"], **kw)  # today's chain
    assert r.seed_index.shape == r.slot_cost.shape == r.slot_class.shape == (B, K) and r.slot_plans.shape == (B, K, d.ndof, T)
    assert (r.n_accepted > 0).sum() >= 6 and ((r.n_accepted > 0) & (r.n_accepted < K)).any() and (r.n_accepted >= K).any()
    for k in ("n_accepted", "seed_cost", "seed_dist", "q_solutions", "err_pos", "err_rot", "ik_cost", "accept"):
        assert getattr(r, k).tobytes() == getattr(one, k).tobytes(), k
    fe = d.frame_index(cfg["link_ee"])
    for b in range(B):
        rows = ref.accepted_rows(n_grasps[b], n, r.accept[b])
        na = len(rows)
        assert na == r.n_accepted[b]
        # slot 0 is today's chain; every ranked slot is the solve of that seed alone; a slot behind them repeats slot 0
        assert r.seed_index[b, 0] == one.seed_index[b] and r.slot_plans[b, 0].tobytes() == one.plans[b].tobytes()
        assert r.slot_cost[b, 0].tobytes() == one.cost[b].tobytes()
        if na:
            order = np.lexsort((r.seed_dist[b, :na], r.seed_cost[b, :na]))[:K]
            assert r.seed_index[b].tolist() == order.tolist() + [-1] * (K - len(order))
            cand = ref.candidates(qc[b], r.q_solutions[b][rows], T, d.param_index, True)
            goals = np.zeros((1, n, 16))
            goals[0, :na] = RT[b][rows].reshape(na, 16)
        for s in range(K):
            if r.seed_index[b, s] < 0:
                assert r.slot_plans[b, s].tobytes() == r.slot_plans[b, 0].tobytes() and r.slot_cost[b, s].tobytes() == r.slot_cost[b, 0].tobytes()
                continue
            Q, dQ, f, _, _ = h.solve_batch(int(b % 2), qc[b:b + 1], goals, na, S, base[b:b + 1], cand[r.seed_index[b, s]][None])
            assert r.slot_plans[b, s].tobytes() == Q[0].tobytes() and r.slot_cost[b, s].tobytes() == f[0].tobytes(), (b, s)
            assert s != r.best_slot[b] or r.dQ[b].tobytes() == dQ[0].tobytes(), (b, s)
        # the choice: the restatement's on the per-slot report, and never after slot 0's
        best, cls, all_cls = mref.select(r.slot_status[b], r.slot_cost[b], r.slot_err_pos[b], r.slot_err_rot[b], r.slot_counts[b],
                                         kw["pos_tol"], kw["rot_tol_deg"], 5)
        assert (r.best_slot[b], r.plan_class[b]) == (best, cls) and r.slot_class[b].tolist() == all_cls, b
        assert best == 0 or mref.slot_before(all_cls[best], r.slot_cost[b, best], best, all_cls[0], r.slot_cost[b, 0], 0), b
        assert (na == 0 or r.seed_index[b, best] >= 0) and (best != 0 or r.dQ[b].tobytes() == one.dQ[b].tobytes()), b
        assert r.plans[b].tobytes() == r.slot_plans[b, best].tobytes() and r.cost[b].tobytes() == r.slot_cost[b, best].tobytes()
        assert np.array_equal(r.counts[b], r.slot_counts[b, best]) and r.status[b] == r.slot_status[b, best]
        # the grasp the plan reached, as a row of the object's grasp list
        if na == 0:
            assert r.goal_row[b] == -1
            continue
        assert 0 <= r.goal_index[b] < na and r.goal_row[b] == rows[r.goal_index[b]] and r.accept[b, r.goal_row[b]]
        Tee = h.eval_fk(r.plans[b][:, T - 1][None])[:, fe]
        ep, er, _ = ref.report(Tee, RT[b, r.goal_row[b]][None], np.zeros(1), 1.0, 1.0, 1.0)
        np.testing.assert_allclose(r.plan_err_pos[b], ep[0], rtol=0, atol=1e-12)  # what the IK report is held to
        np.testing.assert_allclose(r.plan_err_rot[b], er[0], rtol=0, atol=1e-5)
    print("three seeds: best_slot", r.best_slot.tolist(), "plan_class", r.plan_class.tolist(), "slot_class", r.slot_class.tolist(),
          "n_accepted", r.n_accepted.tolist())


def test_chain_with_three_seeds_of_eight_objects_is_eight_single_calls(eight):
    chain, (qc, RT, _, n_grasps, per_obj, base), kw, big = eight["chain"], eight["args"], eight["kw"], eight["three"]
    assert sorted(k for k in vars(big) if not k.startswith("slot_") and k != "accepted_rows") == sorted(set(MULTI_FIELDS) - {"slot_cost", "slot_class", "slot_plans"})
    for b in range(eight["B"]):
        one = chain.plan_objects(qc[b], RT[b:b + 1], RT[b:b + 1], n_grasps[b:b + 1], per_obj[b], base[b], n_seeds=3, **kw)
        for k in MULTI_FIELDS:
            a, c = getattr(one, k), getattr(big, k)[b:b + 1]
            if k in PER_GRASP:
                a, c = a[:, :n_grasps[b]], c[:, :n_grasps[b]]
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(c).tobytes(), (b, k)
