"""GPU: the stream-ordered grasp chain -- gto_solve_ik_pose_batch_device, gto_ik_report_device, gto_seed_goalsets_device
and GraspChain.plan_objects -- against the host-pointer entry points, the numpy restatement (tests/grasp_chain_ref.py)
and the host-composed chain IKSolver.solve_ik_batch -> filter -> GTOPlanner.plan_goalset.  Run the file under a time limit
(timeout -k 10 900 pytest ...) and stop at the first fault."""
import numpy as np
import pytest

import grasp_chain_ref as ref
import grasptrajopt_amd as g
from grasptrajopt_amd import synthetic as syn
from helpers import Problem, cfg_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as gr
    gr.build()
    from grasptrajopt_amd import _capi
    return _capi


def cu(a, dt=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).to("cuda:0")


def dev_empty(shape, dt, fill=None):
    import torch
    t = torch.empty(shape, dtype=dt, device="cuda:0")
    if fill is not None:
        t.fill_(fill)
    return t


def handle_with_scenes(capi, oracle_mod, robot, B, scene_seeds=(5,)):
    prob = Problem(robot, B=B, scene_seed=scene_seeds[0])
    opts = oracle_mod.reference_opts()
    h = capi.SolverHandle(prob.desc, prob.cfg["link_ee"], prob.cfg["link_gripper"], opts, device=0)
    o = oracle_mod.Oracle(prob.desc, prob.cfg["link_ee"], prob.cfg["link_gripper"], opts)
    prob.finish(h.eval_fk)
    for sid, seed in enumerate(scene_seeds):
        sc = prob.scene if sid == 0 else Problem(robot, B=1, scene_seed=seed).scene
        for s in (h, o):
            s.set_scene(sid, sc.c_all, sc.c_obs, sc.shape, sc.origin, sc.res)
    return prob, h, o


def ik_seeds(prob, B, spread=0.3, seed=1):
    rng = np.random.default_rng(seed)
    oi = prob.desc.opt_index
    q0 = np.tile(np.array(prob.qc[0]), (B, 1))
    q0[B // 2:, oi] = prob.qgoal[B // 2:B, 0][:, oi] + rng.uniform(-spread, spread, size=(B - B // 2, len(oi)))
    return q0


# ---------------------------------------------------------------------------------------------- 1. IK
@pytest.mark.parametrize("robot", ["panda", "fetch"])
@pytest.mark.parametrize("collide", [False, True])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_ik_device_is_the_host_call_bit_for_bit(capi, oracle_mod, robot, collide, kind):
    import torch
    from grasptrajopt_amd import utils
    B = 16
    prob, h, _ = handle_with_scenes(capi, oracle_mod, robot, B)
    RT = prob.goals[:, 0].reshape(B, 4, 4)
    goals = {0: RT.reshape(B, 16), 1: np.stack([utils.ik_goal_quaternion(x) for x in RT]), 2: np.stack([utils.ik_goal_rpy(x) for x in RT])}[kind].copy()
    goals[3, 1] = np.nan  # an instance with a NaN goal
    q0, base = ik_seeds(prob, B), np.tile([0.02, -0.01, 0.0], (B, 1))
    sid = np.zeros(B, np.int32) if collide else None
    want = h.solve_ik_pose_batch(kind, None if sid is None else 0, q0, goals, base if collide else None, max_iter=50)
    d_q, d_f = dev_empty((B, prob.desc.ndof), torch.float64), dev_empty((B,), torch.float64)
    d_it, d_st = dev_empty((B,), torch.int32), dev_empty((B,), torch.int32)
    keep = [None if sid is None else cu(sid), cu(q0), cu(goals), cu(base) if collide else None]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    h.solve_ik_pose_batch_device(kind, B, *[None if x is None else x.data_ptr() for x in keep], 50, d_q.data_ptr(), d_f.data_ptr(),
                                 d_it.data_ptr(), d_st.data_ptr(), st.cuda_stream)
    st.synchronize()
    got = [x.cpu().numpy() for x in (d_q, d_f, d_it, d_st)]
    for name, a, b in zip(("q", "cost", "iters", "status"), want, got):
        assert a.tobytes() == b.tobytes(), name
    assert (want[3] != 2).sum() >= B - 1  # the others were solved
    h.close()


def test_ik_device_takes_an_unknown_scene_id_as_numerical(capi, oracle_mod):
    import torch
    B = 4
    prob, h, _ = handle_with_scenes(capi, oracle_mod, "panda", B)
    q0 = ik_seeds(prob, B)
    q0[1, prob.desc.opt_index[0]] = 99.0  # outside the limits: comes back clipped
    sid = np.array([0, 7, -1, 0], np.int32)
    keep = [cu(sid), cu(q0), cu(prob.goals[:, 0].reshape(B, 16)), cu(np.zeros((B, 3)))]
    d_q, d_f = dev_empty((B, prob.desc.ndof), torch.float64), dev_empty((B,), torch.float64)
    d_it, d_st = dev_empty((B,), torch.int32), dev_empty((B,), torch.int32)
    torch.cuda.synchronize()
    h.solve_ik_pose_batch_device(0, B, *[x.data_ptr() for x in keep], 50, d_q.data_ptr(), d_f.data_ptr(), d_it.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    q, f, it, stt = [x.cpu().numpy() for x in (d_q, d_f, d_it, d_st)]
    d = prob.desc
    clipped = q0.copy()
    clipped[:, d.opt_index] = np.clip(q0[:, d.opt_index], d.lower[d.opt_index], d.upper[d.opt_index])
    assert stt[[1, 2]].tolist() == [2, 2] and it[[1, 2]].tolist() == [0, 0] and np.isnan(f[[1, 2]]).all()
    assert np.array_equal(q[[1, 2]], clipped[[1, 2]])
    ref_q, ref_f, ref_it, ref_st = h.solve_ik_batch(0, q0[[0, 3]], prob.goals[[0, 3], 0], np.zeros((2, 3)), max_iter=50)
    assert q[[0, 3]].tobytes() == ref_q.tobytes() and stt[[0, 3]].tolist() == ref_st.tolist()
    h.close()


# ---------------------------------------------------------------------------------------------- 2. report
def widest_gap(values, floor):
    """A threshold in the middle of the widest gap in the upper half of the sorted finite values (so that most instances pass
    and some do not), and the distance from it to the nearest value; above all of them by `floor` if they coincide."""
    v = np.sort(np.asarray(values)[np.isfinite(values)])
    lo = len(v) // 2
    gaps = np.diff(v[lo:])
    if len(gaps) == 0 or gaps.max() <= 0:
        return float(v.max() + floor), float(floor)
    k = lo + int(np.argmax(gaps))
    return float(0.5 * (v[k] + v[k + 1])), float(0.5 * (v[k + 1] - v[k]))


@pytest.mark.parametrize("robot", ["panda", "fetch"])
@pytest.mark.parametrize("collide", [True, False])
def test_report_against_the_numpy_report_of_ik_solver(capi, oracle_mod, robot, collide):
    """err_pos to 1e-12 m, err_rot to 1e-5 degrees, cost to relative 1e-11 against the values IKSolver.solve_ik_batch forms in
    numpy (eval_fk, eval_points); accept equal to the host rule on every instance, with thresholds that the oracle's own FK
    and field lookups put further from every instance than those tolerances."""
    import torch
    B = 32
    prob, h, o = handle_with_scenes(capi, oracle_mod, robot, B)
    d, fe = prob.desc, prob.desc.frame_index(prob.cfg["link_ee"])
    RT = prob.goals[:, 0].reshape(B, 4, 4)
    base = np.tile([0.02, -0.01, 0.0], (B, 1))
    # configurations at different distances from their goals: IK stopped after 0 .. 7 iterations
    q = np.concatenate([h.solve_ik_batch(0, ik_seeds(prob, B)[i:i + 4], RT[i:i + 4].reshape(4, 16), base[i:i + 4], max_iter=i // 4)[0]
                        for i in range(0, B, 4)])
    # the report as IKSolver.solve_ik_batch forms it (grasptrajopt_amd/ik_solver.py:45-49,69-74)
    tf = h.eval_fk(q)[:, fe]
    cost = h.eval_points(0, q, base, use_obs=True, want=("val",))[2].sum(axis=1) if collide else np.zeros(B)
    # thresholds from the oracle's values, clear of every instance
    tf_o = o.eval_fk(q)[:, fe]
    cost_o = o.eval_points(0, q, base, use_obs=True)[2].sum(axis=1) if collide else np.zeros(B)
    ep_o, er_o, _ = ref.report(tf_o, RT, cost_o, 1.0, 1.0, 1.0)
    pos_tol, m_pos = widest_gap(ep_o, 1e-3)
    rot_tol, m_rot = widest_gap(er_o, 1e-2)
    cost_tol, m_cost = widest_gap(cost_o, 1.0)
    assert m_pos > 1e-9 and m_rot > 1e-3 and m_cost > 1e-9 * max(1.0, np.abs(cost_o).max())
    ep, er, acc = ref.report(tf, RT, cost, pos_tol, rot_tol, cost_tol)
    assert np.array_equal(acc, ref.report(tf_o, RT, cost_o, pos_tol, rot_tol, cost_tol)[2])
    if collide:
        assert 0 < acc.sum() < B
    outs = [dev_empty((B,), torch.float64) for _ in range(3)] + [dev_empty((B,), torch.uint8, 9)]
    keep = [cu(np.zeros(B, np.int32)) if collide else None, cu(q), cu(RT.reshape(B, 16)), cu(base) if collide else None]
    torch.cuda.synchronize()
    h.ik_report_device(B, *[None if x is None else x.data_ptr() for x in keep], pos_tol, rot_tol, cost_tol, *[x.data_ptr() for x in outs])
    torch.cuda.synchronize()
    g_ep, g_er, g_cost, g_acc = [x.cpu().numpy() for x in outs]
    print("report", robot, collide, "max |err_pos diff|", np.abs(g_ep - ep).max(), "max |err_rot diff|", np.abs(g_er - er).max(),
          "max rel cost diff", (np.abs(g_cost - cost) / np.maximum(np.abs(cost), 1e-300)).max() if collide else 0.0)
    np.testing.assert_allclose(g_ep, ep, rtol=0, atol=1e-12)
    np.testing.assert_allclose(g_er, er, rtol=0, atol=1e-5)
    np.testing.assert_allclose(g_cost, cost, rtol=1e-11, atol=0)
    assert np.array_equal(g_acc.astype(bool), acc)
    # NULL outputs, a NaN configuration, an instance on its own
    q2 = q.copy()
    q2[5, d.opt_index[1]] = np.nan
    keep[1] = cu(q2)
    outs[3].fill_(9)
    torch.cuda.synchronize()
    h.ik_report_device(B, *[None if x is None else x.data_ptr() for x in keep], pos_tol, rot_tol, cost_tol, None, None, None, outs[3].data_ptr())
    torch.cuda.synchronize()
    a2 = outs[3].cpu().numpy().astype(bool)
    assert not a2[5] and np.array_equal(np.delete(a2, 5), np.delete(acc, 5))
    one = [dev_empty((1,), torch.float64) for _ in range(3)]
    k1 = [cu(np.zeros(1, np.int32)) if collide else None, cu(q[17:18]), cu(RT[17:18].reshape(1, 16)), cu(base[17:18]) if collide else None]
    torch.cuda.synchronize()
    h.ik_report_device(1, *[None if x is None else x.data_ptr() for x in k1], pos_tol, rot_tol, cost_tol, *[x.data_ptr() for x in one], None)
    torch.cuda.synchronize()
    for a, b in zip(one, (g_ep, g_er, g_cost)):
        assert a.cpu().numpy().tobytes() == b[17:18].tobytes()
    h.close()


# ---------------------------------------------------------------------------------------------- 3. seeds
def seed_case(prob, rng, B, n_max):
    d = prob.desc
    oi = d.opt_index
    qc = np.tile(prob.qc[0], (B, 1))
    qc[:, oi] += rng.uniform(-0.05, 0.05, (B, len(oi)))
    qs = np.tile(prob.qc[0], (B, n_max, 1))
    qs[:, :, oi] = rng.uniform(np.maximum(d.lower[oi], -2.5), np.minimum(d.upper[oi], 2.5), (B, n_max, len(oi)))
    goals = rng.standard_normal((B, n_max, 16))
    n_goals = rng.integers(1, n_max + 1, B).astype(np.int32)
    accept = (rng.random((B, n_max)) < 0.7).astype(np.uint8)
    accept[0] = 1
    n_goals[0] = n_max
    accept[1] = 0                      # an instance with an empty mask
    qs[2, 1] = qs[2, 0]                # duplicated solutions: ties in cost and distance
    qs[2, 3] = qs[2, 0]
    accept[2], n_goals[2] = 1, n_max
    qs[3, 0, oi[2]] = np.nan           # a NaN solution, accepted
    accept[3, :2], n_goals[3] = 1, max(2, n_goals[3])
    n_goals[4] = n_max + 3             # read as n_max
    n_goals[5] = 0                     # read as 1
    sid = (np.arange(B) % 2).astype(np.int32)
    base = rng.uniform(-0.03, 0.03, (B, 3))
    return qc, qs, goals, n_goals, accept, sid, base


def run_seeds(h, torch, T, qc, qs, goals, n_goals, accept, sid, base, interpolate, f32):
    B, n_max, ndof = qs.shape
    keep = [cu(sid), cu(qc), cu(goals), cu(n_goals), cu(qs), None if accept is None else cu(accept), cu(base)]
    outs = dict(goals_out=dev_empty((B, n_max, 16), torch.float64, -7.0), n_goals_out=dev_empty((B,), torch.int32, -7),
                n_accepted=dev_empty((B,), torch.int32, -7), Q0=dev_empty((B, ndof, T), torch.float64, -7.0),
                seed_index=dev_empty((B,), torch.int32, -7), seed_cost=dev_empty((B, n_max), torch.float64, -7.0),
                seed_dist=dev_empty((B, n_max), torch.float64, -7.0))
    torch.cuda.synchronize()
    h.seed_goalsets_device(B, n_max, *[None if x is None else x.data_ptr() for x in keep], interpolate, f32,
                           *[x.data_ptr() for x in outs.values()])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b)))) and \
        np.array_equal(np.signbit(a[~np.isnan(a)]), np.signbit(b[~np.isnan(b)]))


@pytest.mark.parametrize("robot", ["panda", "fetch"])
@pytest.mark.parametrize("interpolate", [True, False])
@pytest.mark.parametrize("f32", [True, False])
def test_seeds_against_plan_cost_lexsort_and_the_restatement(capi, oracle_mod, robot, interpolate, f32):
    import torch
    B, n_max = 8, 6
    prob, h, _ = handle_with_scenes(capi, oracle_mod, robot, B, scene_seeds=(5, 9))
    d, T = prob.desc, h.T
    rng = np.random.default_rng(11)
    qc, qs, goals, n_goals, accept, sid, base = seed_case(prob, rng, B, n_max)
    got = run_seeds(h, torch, T, qc, qs, goals, n_goals, accept, sid, base, interpolate, f32)
    for b in range(B):
        score = {}

        def plan_cost(plans, b=b, score=score):
            score["cost"], score["dist"] = h.plan_cost(int(sid[b]), plans, base[b])
            return score["cost"]
        r = ref.seed_goalsets(qc[b], goals[b], n_goals[b], qs[b], accept[b], T, h.opts.standoff_offset, d.param_index, interpolate, f32, plan_cost)
        na = r["n_accepted"]
        assert got["n_accepted"][b] == na and got["n_goals_out"][b] == r["n_goals_out"], b
        assert got["goals_out"][b, :r["n_goals_out"]].tobytes() == r["goals_out"].tobytes(), b
        assert (got["goals_out"][b, r["n_goals_out"]:] == -7.0).all() and (got["seed_cost"][b, na:] == -7.0).all(), b  # untouched
        assert got["Q0"][b].tobytes() == r["Q0"].tobytes() or same_bits(got["Q0"][b], r["Q0"]), b
        if na == 0:
            assert got["seed_index"][b] == -1
            continue
        # bit-equal to gto_plan_cost of the host-built candidates (a NaN distance is a NaN on both sides)
        assert got["seed_cost"][b, :na].tobytes() == score["cost"].tobytes(), b
        assert same_bits(got["seed_dist"][b, :na], score["dist"]), (b, got["seed_dist"][b, :na], score["dist"])
        assert same_bits(r["seed_dist"], score["dist"])
        assert got["seed_index"][b] == int(np.lexsort((score["dist"], score["cost"]))[0]) == r["seed_index"], b
    assert got["n_accepted"][1] == 0 and got["n_accepted"][2] == n_max and got["seed_index"][2] == int(np.lexsort((got["seed_dist"][2], got["seed_cost"][2]))[0])
    assert np.isnan(got["seed_dist"][3, 0])
    # accept = NULL: every row counts
    allg = run_seeds(h, torch, T, qc, qs, goals, n_goals, None, sid, base, interpolate, f32)
    ones = run_seeds(h, torch, T, qc, qs, goals, n_goals, np.ones_like(accept), sid, base, interpolate, f32)
    for k in allg:
        assert allg[k].tobytes() == ones[k].tobytes(), k
    # any position in any batch: reversed, and one instance on its own
    rev = run_seeds(h, torch, T, *[x[::-1].copy() for x in (qc, qs, goals, n_goals, accept, sid, base)], interpolate, f32)
    for k in got:
        assert rev[k][::-1].tobytes() == got[k].tobytes(), k
    one = run_seeds(h, torch, T, *[x[4:5].copy() for x in (qc, qs, goals, n_goals, accept, sid, base)], interpolate, f32)
    for k in got:
        assert one[k].tobytes() == got[k][4:5].tobytes(), k
    h.close()


def test_entry_points_validate_on_the_host(capi, oracle_mod):
    import torch
    prob, h, _ = handle_with_scenes(capi, oracle_mod, "panda", 2)
    x = dev_empty((64,), torch.float64, 0.0).data_ptr()
    h.seed_goalsets_device(0, 1, None, None, None, None, None, None, None, 1, 1)  # B = 0: no launch, no argument looked at
    h.ik_report_device(0, None, None, None, None, 0.01, 5.0, 5.0)
    h.solve_ik_pose_batch_device(0, 0, None, None, None, None, 50, None)
    with pytest.raises(capi.GTOError, match=r"\(-1\)"):
        h.seed_goalsets_device(1, 0, x, x, x, x, x, None, x, 1, 1)
    with pytest.raises(capi.GTOError, match=r"\(-1\)"):
        h.seed_goalsets_device(1, 1, x, x, x, x, None, None, x, 1, 1)
    with pytest.raises(capi.GTOError, match=r"\(-1\)"):
        h.ik_report_device(1, x, x, x, None, 0.01, 5.0, 5.0)
    with pytest.raises(capi.GTOError, match=r"\(-1\)"):
        h.solve_ik_pose_batch_device(0, 1, x, x, x, None, 50, x)
    with pytest.raises(capi.GTOError, match=r"\(-1\)"):
        h.solve_ik_pose_batch_device(3, 1, None, x, x, None, 50, x)
    h.close()
    from helpers import limit_robot
    desc, ee = limit_robot("chain", n_opt=9)
    hw = capi.SolverHandle(desc, ee, ee, device=0)
    for call in (lambda: hw.seed_goalsets_device(1, 1, x, x, x, x, x, None, x, 1, 1), lambda: hw.ik_report_device(1, None, x, x, None, 0.01, 5.0, 5.0),
                 lambda: hw.solve_ik_pose_batch_device(0, 1, None, x, x, None, 50, x)):
        with pytest.raises(capi.GTOError, match=r"\(-4\).*eight optimised joints"):
            call()
    hw.close()


# ---------------------------------------------------------------------------------------------- 4. the chain
def chain_setup(robot_name, n_goals, seed):
    rng = np.random.default_rng(seed)
    cfg = cfg_of(robot_name)
    robot = g.GTORobotModel(desc=g.load_builtin(robot_name), time_derivs=[0, 1], param_joints=cfg["param_joints"],
                            collision_link_names=cfg["collision_link_names"], device=0)
    fetch = robot_name.startswith("fetch")
    lo, hi = ([0.3, -0.4, 0.4], [0.9, 0.4, 1.0]) if fetch else ([0.25, -0.45, -0.02], [0.8, 0.45, 0.35])
    robot.setup_points_field(rng.uniform(lo, hi, size=(400, 3)))
    wp = robot.workspace_points
    tz = 0.45 if fetch else 0.0
    box_c = np.array([0.6, 0.1, tz + 0.1])
    fields = []
    for shift in (0.0, 0.12):  # two scenes: the box moved
        d_table = wp[:, 2] - tz
        qd = np.abs(wp - (box_c + [0.0, shift, 0.0])) - np.array([0.06, 0.06, 0.1])
        d_box = np.linalg.norm(np.maximum(qd, 0), axis=1) + np.minimum(qd.max(axis=1), 0)
        fields.append((syn.sdf_cost_map(np.minimum(d_table, d_box), epsilon=0.06).astype(np.float32),
                       syn.sdf_cost_map(np.minimum(d_table, d_box + 0.03), epsilon=0.06).astype(np.float32)))
    h = robot._util_handle()
    zl = (0.6, 1.1) if fetch else (0.15, 0.6)
    RT, _ = syn.make_goals(robot.desc, h.eval_fk, cfg["link_ee"], n_goals, seed=seed, zlim=zl)
    return cfg, robot, fields, RT


def host_chain(robot, cfg, qc, ik_RT, plan_RT, fields, base, interpolate, pos_tol, rot_tol, cost_tol, max_iter):
    """The chain as the host composes it: IKSolver.solve_ik_batch, the driver's filter (:262-269), GTOPlanner.plan_goalset with
    the float32 q_solutions."""
    ik = g.IKSolver(robot, cfg["link_ee"], cfg["link_gripper"], collision_avoidance=True)
    ik.max_iter = IK_ITERS
    q, ep, er, cost, it, st = ik.solve_ik_batch(qc, ik_RT, fields[1], base)
    found = (ep < pos_tol) & (er < rot_tol) & (cost < cost_tol)
    out = dict(q=q, err_pos=ep, err_rot=er, ik_cost=cost, accept=found)
    if not found.any():
        return out
    planner = g.GTOPlanner(robot, cfg["link_ee"], cfg["link_gripper"], standoff_distance=-0.1, standoff_offset=-10)
    planner.max_iter = max_iter
    q_solutions = q.T.astype(np.float32)[:, found]
    plan, dQ, f = planner.plan_goalset(qc, plan_RT[found], fields[0], fields[1], base, q_solutions, use_standoff=True,
                                       axis_standoff=cfg["axis_standoff"], interpolate=interpolate)
    out.update(plan=plan, dQ=dQ, f=f, seed_index=planner.seed_index, iters=planner.solver.number_of_iterations())
    return out


IK_ITERS = 4  # IK stopped early: the candidates end at different distances from their goals


def chain_thresholds(robot, cfg, qc, ik_RT, fields, base):
    """A position threshold in the widest gap of the host's own report, so that some grasps pass and some do not; the other
    two thresholds out of every grasp's way."""
    ik = g.IKSolver(robot, cfg["link_ee"], cfg["link_gripper"], collision_avoidance=True)
    ik.max_iter = IK_ITERS
    _, ep, er, cost, _, _ = ik.solve_ik_batch(qc, ik_RT, fields[1], base)
    pos_tol, m = widest_gap(ep, 1e-3)
    assert m > 1e-9  # three orders above the 1e-12 the report is held to
    return pos_tol, 360.0, float(np.abs(cost).max()) * 2.0 + 1.0


@pytest.mark.parametrize("robot_name", ["panda", "fetch"])
@pytest.mark.parametrize("interpolate", [True, False])
def test_chain_on_one_object_is_the_host_composed_chain(robot_name, interpolate):
    from grasptrajopt_amd.grasp_chain import GraspChain
    n = 6
    cfg, robot, fields, RT = chain_setup(robot_name, n, seed=21)
    qc = np.array(cfg["default_pose"], dtype=np.float64)
    base = np.array([0.01, -0.02, 0.0])
    S = syn.standoff_pose(-0.1, cfg["axis_standoff"])
    ik_RT = RT @ S  # the shelf driver: IK to the standoff pose, the plan to the grasp (:256-259)
    pos_tol, rot_tol, cost_tol = chain_thresholds(robot, cfg, qc, ik_RT, fields[0], base)
    want = host_chain(robot, cfg, qc, ik_RT, RT, fields[0], base, interpolate, pos_tol, rot_tol, cost_tol, 30)
    assert 0 < want["accept"].sum() < n
    chain = GraspChain(robot, cfg["link_ee"], cfg["link_gripper"], standoff_distance=-0.1, standoff_offset=-10)
    chain.max_iter, chain.ik_max_iter = 30, IK_ITERS
    dpc = g.DepthPointCloud(*syn.wall_scene()[:3], target_mask=syn.wall_scene()[3], threshold=1.5)
    obs = dpc.observation()
    vmax, amax = np.full(robot.ndof, 2.0), np.full(robot.ndof, 4.0)
    r = chain.plan_objects(qc, ik_RT[None], RT[None], [n], fields[0], base, axis_standoff=cfg["axis_standoff"], interpolate=interpolate,
                           pos_tol=pos_tol, rot_tol_deg=rot_tol, ik_collision_threshold=cost_tol, observation=obs,
                           retime=dict(vmax=vmax, amax=amax))
    assert r.q_solutions.dtype == np.float32 and r.q_solutions[0].tobytes() == want["q"].astype(np.float32).tobytes()
    np.testing.assert_allclose(r.err_pos[0], want["err_pos"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(r.err_rot[0], want["err_rot"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(r.ik_cost[0], want["ik_cost"], rtol=1e-11, atol=0)
    assert np.array_equal(r.accept[0], want["accept"]) and r.n_accepted[0] == want["accept"].sum()
    assert r.seed_index[0] == want["seed_index"]
    assert r.plans[0].tobytes() == want["plan"].tobytes() and r.dQ[0].tobytes() == want["dQ"].tobytes()
    assert r.cost.tobytes() == want["f"].tobytes() and r.iters[0] == want["iters"]
    h = robot._util_handle()
    assert np.array_equal(r.counts, h.check_plans(obs, r.plans, base))
    rt = h.retime_batch(r.plans, vmax, amax)
    assert r.durations.tobytes() == rt["duration"].tobytes() and np.array_equal(r.retime_status, rt["status"])
    # no feasible grasp: the solve from the constant seed to every goal, and the caller is told
    r0 = chain.plan_objects(qc, ik_RT[None], RT[None], [n], fields[0], base, axis_standoff=cfg["axis_standoff"], interpolate=interpolate,
                            pos_tol=pos_tol, rot_tol_deg=rot_tol, ik_collision_threshold=-1.0)
    assert r0.n_accepted[0] == 0 and r0.seed_index[0] == -1 and not r0.accept.any()
    planner = g.GTOPlanner(robot, cfg["link_ee"], cfg["link_gripper"], standoff_distance=-0.1, standoff_offset=-10)
    planner.max_iter = 30
    plan0, _, _ = planner.plan_goalset(qc, RT, fields[0][0], fields[0][1], base, None, use_standoff=True, axis_standoff=cfg["axis_standoff"])
    assert r0.plans[0].tobytes() == plan0.tobytes()
    chain.close()
    robot.close()


def test_chain_of_eight_objects_over_two_scenes_is_eight_single_calls():
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
    # the host's own report of every candidate (IK stopped early, as in the one-object test): a position threshold in its
    # widest gap, so that some grasps pass and some do not; the other two thresholds out of every grasp's way
    ik = g.IKSolver(robot, cfg["link_ee"], cfg["link_gripper"], collision_avoidance=True)
    ik.max_iter = IK_ITERS
    host = [ik.solve_ik_batch(qc[b], RT[b], per_obj[b][1], base[b]) for b in range(B)]
    ep, er, cost = (np.stack([h_[i] for h_ in host]) for i in (1, 2, 3))
    counted = np.arange(n)[None, :] < n_grasps[:, None]
    pos_tol, margin = widest_gap(ep[counted], 1e-3)
    assert margin > 1e-9  # three orders above the 1e-12 the report is held to
    cost_tol = float(np.abs(cost).max()) * 2.0 + 1.0
    print("eight objects: host err_pos", np.sort(ep[counted]), "pos_tol", pos_tol, "max err_rot", er.max(), "max cost", cost.max())
    chain = GraspChain(robot, cfg["link_ee"], cfg["link_gripper"])
    chain.max_iter, chain.ik_max_iter = 30, IK_ITERS
    kw = dict(axis_standoff=cfg["axis_standoff"], pos_tol=pos_tol, rot_tol_deg=360.0, ik_collision_threshold=cost_tol)
    big = chain.plan_objects(qc, RT, RT, n_grasps, per_obj, base, **kw)
    want = (ep < pos_tol) & counted
    assert np.array_equal(big.accept & counted, want) and 0 < want.sum() < counted.sum()
    assert np.array_equal(big.n_accepted, want.sum(axis=1))
    for b in range(B):
        one = chain.plan_objects(qc[b], RT[b:b + 1], RT[b:b + 1], n_grasps[b:b + 1], per_obj[b], base[b], **kw)
        for k in ("plans", "dQ", "cost", "iters", "status", "n_accepted", "seed_index", "q_solutions", "err_pos", "err_rot", "ik_cost", "accept"):
            a, c = getattr(one, k), getattr(big, k)[b:b + 1]
            if k in ("q_solutions", "err_pos", "err_rot", "ik_cost", "accept"):  # rows behind n_grasps are padding
                a, c = a[:, :n_grasps[b]], c[:, :n_grasps[b]]
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(c).tobytes(), (b, k)
    chain.close()
    robot.close()
