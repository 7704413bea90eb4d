"""gto_solve_ik_pose_batch on the MI355X: the position + quaternion / roll-pitch-yaw goals of
gto/ik_solver_quaternion.py and gto/ik_solver_rpy.py inside k_ik_solve, against the numpy restatement
(tests/ik_pose_ref.py), the oracle's collision term, SciPy's L-BFGS-B and the existing point-goal IK."""
import numpy as np
import pytest

import ik_pose_ref as ref
from grasptrajopt_amd import synthetic as syn
from helpers import Problem

pytestmark = pytest.mark.gpu
KINDS = [ref.GTO_IK_GOAL_QUATERNION, ref.GTO_IK_GOAL_RPY]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


def make_pair(capi, oracle_mod, prob, **opt_kw):
    opts = oracle_mod.reference_opts(**opt_kw)
    h = capi.SolverHandle(prob.desc, prob.cfg["link_ee"], prob.cfg["link_gripper"], opts, device=0)
    o = oracle_mod.Oracle(prob.desc, prob.cfg["link_ee"], prob.cfg["link_gripper"], opts)
    prob.finish(h.eval_fk)
    h.set_scene(*prob.scene_args())
    o.set_scene(*prob.scene_args())
    return h, o, opts


def goal_vectors(kind, RTs):
    from grasptrajopt_amd import utils
    conv = utils.ik_goal_quaternion if kind == ref.GTO_IK_GOAL_QUATERNION else utils.ik_goal_rpy
    return np.stack([conv(RT) for RT in np.asarray(RTs).reshape(-1, 4, 4)])


def seeds(prob, B, spread=0.3, seed=1):
    rng = np.random.default_rng(seed)
    oi = prob.desc.opt_index
    q0 = np.tile(np.array(prob.qc[0]), (B, 1))
    q0[B // 2:, oi] = prob.qgoal[B // 2:B, 0][:, oi] + rng.uniform(-spread, spread, size=(B - B // 2, len(oi)))
    return q0


# ------------------------------------------------------------------------------------------ 1. kind 0
@pytest.mark.parametrize("robot", ["panda", "fetch"])
@pytest.mark.parametrize("collide", [False, True])
def test_kind0_is_gto_solve_ik_batch_bit_for_bit(capi, oracle_mod, robot, collide):
    prob = Problem(robot, B=16, scene_seed=5)
    h, _, _ = make_pair(capi, oracle_mod, prob)
    q0, sid = seeds(prob, 16), (0 if collide else None)
    a = h.solve_ik_batch(sid, q0, prob.goals[:, 0], prob.base, max_iter=50)
    b = h.solve_ik_pose_batch(0, sid, q0, prob.goals[:, 0], prob.base, max_iter=50)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    h.close()


# ------------------------------------------------------------------------------------------ 2. objective at the seed
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("collide,grad_mode", [(False, 0), (True, 0), (True, 1)])
@pytest.mark.parametrize("robot", ["panda", "fetch"])
def test_cost_at_seed_is_pose_term_plus_collision(capi, oracle_mod, robot, kind, collide, grad_mode):
    prob = Problem(robot, B=12, scene_seed=5)
    h, o, opts = make_pair(capi, oracle_mod, prob, grad_mode=grad_mode)
    q0 = seeds(prob, 12)
    g = goal_vectors(kind, prob.goals[:, 0])
    sid = 0 if collide else None
    q, cost, it, st = h.solve_ik_pose_batch(kind, sid, q0, g, prob.base, max_iter=0)
    assert (it == 0).all() and (st == ref.GTO_STATUS_MAX_ITER).all()
    oi, d = prob.desc.opt_index, prob.desc
    qc = q0.copy()
    qc[:, oi] = np.clip(q0[:, oi], d.lower[oi], d.upper[oi])
    np.testing.assert_array_equal(q, qc)
    fe = d.frame_index(prob.cfg["link_ee"])
    fr = o.eval_fk(qc)[:, fe]
    want = np.array([ref.pose_term(kind, fr[b], g[b]) for b in range(12)])
    if collide:
        _, _, val, _ = o.eval_points(0, qc, prob.base, use_obs=True)
        want = want + opts.w_obstacle * val.sum(axis=1)
    np.testing.assert_allclose(cost, want, rtol=1e-10, atol=1e-14)
    h.close()


# ------------------------------------------------------------------------------------------ 3. lock-step
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("robot", ["panda", "fetch"])
def test_lockstep_with_numpy_restatement(capi, oracle_mod, robot, kind):
    B = 32
    prob = Problem(robot, B=B, scene_seed=5)
    h, o, opts = make_pair(capi, oracle_mod, prob)
    q0 = seeds(prob, B)
    g = goal_vectors(kind, prob.goals[:, 0])
    q, cost, it, st = h.solve_ik_pose_batch(kind, None, q0, g, None, max_iter=50)
    for b in range(B):
        p = ref.PoseProblem(o, prob.desc, prob.cfg["link_ee"], kind, q0[b], g[b])
        qr, fr, itr, str_ = ref.solve(p, q0[b], opts, 50)
        assert (it[b], st[b]) == (itr, str_), (b, it[b], itr, st[b], str_)
        np.testing.assert_allclose(q[b], qr, rtol=0, atol=1e-9, err_msg=f"instance {b}")
        np.testing.assert_allclose(cost[b], fr, rtol=1e-10, atol=1e-15)
    h.close()


# ------------------------------------------------------------------------------------------ 4. against L-BFGS-B
@pytest.mark.parametrize("kind", KINDS)
def test_with_collision_ends_where_lbfgsb_ends(capi, oracle_mod, kind):
    from independent import lbfgsb_fd
    B = 8
    prob = Problem("panda", B=B, scene_seed=5)
    h, o, opts = make_pair(capi, oracle_mod, prob, tol_rel_f=1e-14)
    q0 = seeds(prob, B, spread=0.15)
    g = goal_vectors(kind, prob.goals[:, 0])
    q, cost, it, st = h.solve_ik_pose_batch(kind, 0, q0, g, prob.base, max_iter=200)
    d, oi = prob.desc, prob.desc.opt_index
    fe = d.frame_index(prob.cfg["link_ee"])
    lo, hi = d.lower[oi], d.upper[oi]
    better = 0
    for b in range(B):
        def fbatch(X, b=b):
            Q = np.repeat(q[b:b + 1], len(X), 0)
            Q[:, oi] = X
            fr = o.eval_fk(Q)[:, fe]
            _, _, val, _ = o.eval_points(0, Q, prob.base[b], use_obs=True)
            return np.array([ref.pose_term(kind, fr[i], g[b]) for i in range(len(X))]) + opts.w_obstacle * val.sum(axis=1)
        np.testing.assert_allclose(fbatch(q[b:b + 1, oi])[0], cost[b], rtol=1e-9, atol=1e-13)
        r2 = lbfgsb_fd(fbatch, q[b, oi], lo, hi)
        if r2.fun >= cost[b] * (1 - 1e-6) - 1e-10:
            better += 1
    assert better >= B - 1, f"L-BFGS-B improved on {B - better} of {B} answers"
    h.close()


# ------------------------------------------------------------------------------------------ 5. reach
@pytest.mark.parametrize("robot", ["panda", "fetch"])
def test_reach_of_each_kind(capi, oracle_mod, robot):
    B = 256
    prob = Problem(robot, B=4, scene_seed=5)
    h, o, _ = make_pair(capi, oracle_mod, prob)
    d, cfg = prob.desc, prob.cfg
    zl = (0.55, 1.2) if robot == "fetch" else (0.08, 0.7)
    RT, _ = syn.make_goals(d, h.eval_fk, cfg["link_ee"], B, seed=11, zlim=zl)
    q0 = np.tile(prob.qc[0], (B, 1))
    fe = d.frame_index(cfg["link_ee"])
    share = {}
    for kind in (0, 1, 2):
        goals = RT.reshape(B, 16) if kind == 0 else goal_vectors(kind, RT)
        q, cost, it, st = h.solve_ik_pose_batch(kind, None, q0, goals, None, max_iter=50)
        T = h.eval_fk(q)[:, fe]
        ep = np.linalg.norm(T[:, :3, 3] - RT[:, :3, 3], axis=1)
        ca = (np.einsum("bij,bij->b", RT[:, :3, :3], T[:, :3, :3]) - 1.0) / 2.0
        er = np.degrees(np.arccos(np.clip(ca, -1, 1)))
        share[kind] = float(np.mean((ep < 0.01) & (er < 5.0)))
        assert np.isfinite(q).all() and np.isfinite(cost).all()
    print(f"{robot}: share within 1 cm and 5 deg: points {share[0]:.3f} quaternion {share[1]:.3f} rpy {share[2]:.3f}")
    assert share[1] >= share[0] - 0.05
    h.close()


# ------------------------------------------------------------------------------------------ 6. clamp, cut, NaN
def test_rpy_at_clamp_and_yaw_cut_and_nan_goals(capi, oracle_mod):
    prob = Problem("fetch", B=8, scene_seed=5)
    h, o, _ = make_pair(capi, oracle_mod, prob)
    from conftest import golden
    fx = golden("ik_pose.npz")
    qs = fx["fetch_q"][fx["fetch_kind"] > 0]
    B = len(qs)
    q0 = np.tile(prob.qc[0], (B, 1))
    g = np.concatenate([fx["fetch_pos"][fx["fetch_kind"] > 0], fx["fetch_rpy"][fx["fetch_kind"] > 0]], axis=1)
    g_cut = g.copy()
    g_cut[:, 5] = np.where(np.arange(B) % 2 == 0, np.pi - 1e-9, -np.pi + 1e-9)  # yaw goals on both sides of the cut
    for goals in (g, g_cut):
        q, cost, it, st = h.solve_ik_pose_batch(ref.GTO_IK_GOAL_RPY, 0, q0, goals, np.zeros((B, 3)), max_iter=50)
        assert np.isfinite(q).all() and np.isfinite(cost).all()
        assert np.isin(st, [ref.GTO_STATUS_CONVERGED, ref.GTO_STATUS_MAX_ITER]).all()
    # seeds on the clamp itself
    q, cost, it, st = h.solve_ik_pose_batch(ref.GTO_IK_GOAL_RPY, None, qs, g_cut, None, max_iter=50)
    assert np.isfinite(q).all() and np.isfinite(cost).all()
    assert np.isin(st, [ref.GTO_STATUS_CONVERGED, ref.GTO_STATUS_MAX_ITER]).all()
    # non-finite goals: at once NUMERICAL with 0 iterations (the header's rule), never CONVERGED; neighbours untouched
    q0 = seeds(prob, 8)
    for kind in KINDS:
        goals = goal_vectors(kind, prob.goals[:, 0])
        clean = h.solve_ik_pose_batch(kind, 0, q0, goals, prob.base, max_iter=50)
        bad = goals.copy()
        bad[1, 0] = np.nan
        bad[3, 4] = np.nan
        bad[5, 2] = np.inf
        q, cost, it, st = h.solve_ik_pose_batch(kind, 0, q0, bad, prob.base, max_iter=50)
        for b in (1, 3, 5):
            assert st[b] == ref.GTO_STATUS_NUMERICAL and it[b] == 0
        ok = [0, 2, 4, 6, 7]
        for x, y in zip(clean, (q, cost, it, st)):
            assert x[ok].tobytes() == y[ok].tobytes()
    h.close()


# ------------------------------------------------------------------------------------------ 7. errors
def test_errors(capi, oracle_mod):
    prob = Problem("panda", B=4, scene_seed=5)
    h, _, _ = make_pair(capi, oracle_mod, prob)
    q0 = seeds(prob, 4)
    g = goal_vectors(1, prob.goals[:, 0])
    for kind in (-1, 3, 7):
        with pytest.raises(capi.GTOError) as e:
            h.solve_ik_pose_batch(kind, None, q0, np.zeros((4, 6)), None)
        assert e.value.args and "goal kind" in str(e.value)
    with pytest.raises(capi.GTOError, match="scene"):
        h.solve_ik_pose_batch(1, 7, q0, g, prob.base)
    h.close()
    from grasptrajopt_amd.robot_desc import load_builtin, with_planar_base
    from helpers import cfg_of
    cfg = cfg_of("fetch")
    d = with_planar_base(load_builtin("fetch"))
    assert len(d.opt_index) > 8
    hm = capi.SolverHandle(d, cfg["link_ee"], cfg["link_gripper"], device=0)
    with pytest.raises(capi.GTOError, match="eight"):
        hm.solve_ik_pose_batch(2, None, np.zeros((2, d.ndof)), np.zeros((2, 6)), None)
    hm.close()


# ------------------------------------------------------------------------------------------ 8. batch independence
@pytest.mark.parametrize("kind", KINDS)
def test_large_batch_matches_single_calls(capi, oracle_mod, kind):
    B = 4096
    prob = Problem("panda", B=8, scene_seed=5)
    h, _, _ = make_pair(capi, oracle_mod, prob)
    d, cfg = prob.desc, prob.cfg
    RT, qg = syn.make_goals(d, h.eval_fk, cfg["link_ee"], 64, seed=3)
    rng = np.random.default_rng(4)
    idx = rng.integers(0, 64, size=B)
    g = goal_vectors(kind, RT)[idx]
    q0 = np.tile(prob.qc[0], (B, 1))
    oi = d.opt_index
    q0[:, oi] += rng.uniform(-0.2, 0.2, size=(B, len(oi)))
    base = np.tile(prob.base[0], (B, 1))
    big = h.solve_ik_pose_batch(kind, 0, q0, g, base, max_iter=50)
    for b in rng.choice(B, size=12, replace=False):
        one = h.solve_ik_pose_batch(kind, 0, q0[b:b + 1], g[b:b + 1], base[b:b + 1], max_iter=50)
        for x, y in zip(big, one):
            assert x[b:b + 1].tobytes() == y.tobytes()
    h.close()


# ------------------------------------------------------------------------------------------ 9. drop-in modules
@pytest.mark.parametrize("modname", ["ik_solver_quaternion", "ik_solver_rpy"])
def test_drop_in_modules(capi, modname):
    """The reference's constructor / setup_optimization / solve_ik on Panda with the cost field of a DepthPointCloud
    scene: the reference tuple, err_pos / err_rot recomputed from FK, cost = compute_plan_cost of the one-column plan."""
    import importlib
    import grasptrajopt_amd as g
    from grasptrajopt_amd import utils
    from helpers import cfg_of
    mod = importlib.import_module(f"grasptrajopt_amd.{modname}")
    cfg = cfg_of("panda")
    robot = g.GTORobotModel(desc=g.load_builtin("panda"), time_derivs=[0, 1], param_joints=cfg["param_joints"],
                            collision_link_names=cfg["collision_link_names"], device=0)
    rng = np.random.default_rng(0)
    robot.setup_points_field(rng.uniform([0.25, -0.45, -0.02], [0.8, 0.45, 0.35], size=(400, 3)))
    H, W = 60, 80
    K = np.array([[70.0, 0, 40.0], [0, 70.0, 30.0], [0, 0, 1.0]])
    cam = np.eye(4)
    cam[:3, :3] = np.array([[0, -1.0, 0], [-1.0, 0, 0], [0, 0, -1.0]])
    cam[:3, 3] = [0.5, 0.0, 1.2]
    depth = np.full((H, W), 1.2, dtype=np.float32)
    depth[20:40, 30:50] = 0.9
    sdf = g.DepthPointCloud(depth, K, cam).get_sdf_cost(robot.workspace_points)
    ik = mod.IKSolver(robot, cfg["link_ee"], cfg["link_gripper"])
    ik.setup_optimization()
    fe = robot.desc.frame_index(cfg["link_ee"])
    RT, _ = syn.make_goals(robot.desc, ik._handle.eval_fk, cfg["link_ee"], 3, seed=2)
    qc = np.array(cfg["default_pose"])
    for i in range(3):
        out = ik.solve_ik(qc.reshape(-1, 1), RT[i], sdf, [0.0, 0.0, 0.0])
        assert len(out) == 4
        q, err_pos, err_rot, cost = out
        assert q.shape == (robot.ndof,)
        T = ik.solve_fk(q)
        np.testing.assert_allclose(T, ik._handle.eval_fk(q[None])[0, fe], atol=0)
        assert abs(err_pos - np.linalg.norm(RT[i, :3, 3] - T[:3, 3])) < 1e-12
        dq = np.dot(utils.mat2quat(RT[i, :3, :3]), utils.mat2quat(T[:3, :3]))
        assert abs(err_rot - np.degrees(np.arccos(np.clip(2 * dq * dq - 1, -1, 1)))) < 1e-9
        Tn = robot._util_handle().T  # compute_plan_cost sums over the columns of a plan of the handle's length
        c_plan, _ = robot.compute_plan_cost(np.repeat(q[:, None], Tn, 1), sdf, [0.0, 0.0, 0.0])
        np.testing.assert_allclose(cost * Tn, c_plan, rtol=1e-9, atol=1e-9)
    robot.close()
