"""GPU: the solver at the capacity include/gto_solver.h advertises, against the FP64 oracle (oracle/gto_oracle.c).

Robots (tests/helpers.limit_robot), 32 frames and 32 collision links each, 64 points per link (32 chunks):
  chain-8 / chain-9 / chain-16   a serial chain of depth 31, 31 actuated joints, the end effector at the bottom
  bushy-8 / bushy-9 / bushy-16   a chain of n_opt + 3 frames and side branches hung on random earlier frames
  forked-8                       the same chain with three serial side branches on three chain frames
Size-dependent paths each one crosses (helpers.limit_paths; asserted below):
  * kernel width: n_opt 8 runs the 8-wide obstacle and step kernels (k_obstacle_gram<8,*>, k_lm_step<4,1> / <8,4>),
    n_opt 9 and 16 the 16-wide ones (k_obstacle_gram<16,*>, k_lm_step_wide<16>);
  * obstacle workgroup size: with 32 links of 32 chunks, eight waypoints per workgroup do not fit the LDS; gto_create
    sizes these robots for fewer (the 8-wide ones were refused before);
  * broad-phase tail of k_lm_step<4,1> (8-wide only, launches with more than GTO_FEW_INSTANCES instances in flight): its
    tables have 4 F = 128 frame rows plus the sphere image, more than the 128 GTO_PB_PRE rows waves 2-3 stage: every one of
    these robots fetches the remaining rows in the tail; 31 - n_opt (chain) or 15-23 (bushy, forked) parameter joints
    over T - 2 waypoints are more than the 256 staged joint values;
  * parked frames (RobotDev::n_xst): none on the chain, three on the forked tree, seven or more on the bushy one; the
    tail has four register slots, so the tail runs on chain-8 and forked-8 and is off on bushy-8 (more than four).
The largest horizon gto_create accepts is T = 96 (GTO_MAX_T) for every one of them; each runs at T = 50 and T = 96.

Goal sets larger than one wave: goal_terms_wave gives each of the 64 lanes every 64th goal; the arg-min must be the
first minimum over both strides (optas.mmin)."""
import numpy as np
import pytest

from grasptrajopt_amd import synthetic as syn
from helpers import cfg_of, limit_paths, limit_robot

pytestmark = pytest.mark.gpu

ROBOTS = [("chain", 8), ("chain", 9), ("chain", 16), ("bushy", 8), ("bushy", 9), ("bushy", 16), ("forked", 8)]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


def _field(rng, n=44, res=0.1, origin=(-2.2, -2.2, -2.2)):
    """Cost values in a slab (x > 0.1) and zeros elsewhere: some waypoint groups meet the field, some settle."""
    c_all = (0.03 * rng.random(n ** 3) * (rng.random(n ** 3) < 0.35)).astype(np.float32).reshape(n, n, n)
    c_obs = (0.03 * rng.random(n ** 3) * (rng.random(n ** 3) < 0.25)).astype(np.float32).reshape(n, n, n)
    x = origin[0] + res * np.arange(n)
    c_all[x < 0.1] = 0.0
    c_obs[x < 0.1] = 0.0
    return c_all.reshape(-1), c_obs.reshape(-1), (n, n, n), origin, res


class LimitCase:
    def __init__(self, capi, oracle_mod, kind, n_opt, T, B=6, n_max=5, seed=0, env=None, max_iter=15):
        self.desc, self.ee = limit_robot(kind, n_opt=n_opt, seed=seed)
        d = self.desc
        self.T, self.B = T, B
        self.opts = oracle_mod.reference_opts(T=T, standoff_offset=-max(2, T // 5), max_iter=max_iter)
        self.h = capi.SolverHandle(d, self.ee, self.ee, self.opts, device=0, n_gripper_points=40)
        self.o = oracle_mod.Oracle(d, self.ee, self.ee, self.opts, n_gripper_points=40)
        self.nt = self.o.usable_cores()
        rng = np.random.default_rng(1000 + 17 * n_opt + T + seed)
        self.scene = _field(rng)
        self.h.set_scene(0, *self.scene)
        self.o.set_scene(0, *self.scene)
        lo, hi = d.lower, d.upper
        self.qc = rng.uniform(0.3 * lo, 0.3 * hi, size=(B, d.ndof))
        qg = rng.uniform(0.8 * lo, 0.8 * hi, size=(B, n_max, d.ndof))
        qg[:, :, d.param_index] = self.qc[:, None, d.param_index]
        self.goals = self.o.eval_fk(qg.reshape(-1, d.ndof))[:, d.frame_index(self.ee)].reshape(B, n_max, 16)
        self.n_goals = rng.integers(1, n_max + 1, size=B).astype(np.int32)
        self.n_goals[0] = n_max
        self.S = syn.standoff_pose(-0.05, "z")
        self.base = rng.uniform(-0.05, 0.05, size=(B, 3))
        self.Q0 = np.stack([syn.make_seed(self.qc[b], qg[b, 0], T, d.param_index) for b in range(B)])
        self.rng = rng

    def solve_args(self):
        return (0, self.qc, self.goals, self.n_goals, self.S, self.base, self.Q0)

    def close(self):
        self.h.close()


@pytest.mark.parametrize("T", [50, 96])
@pytest.mark.parametrize("kind,n_opt", ROBOTS)
def test_limit_robot_pieces_match_oracle(capi, oracle_mod, kind, n_opt, T):
    c = LimitCase(capi, oracle_mod, kind, n_opt, T)
    d, h, o = c.desc, c.h, c.o
    assert (d.n_frames, d.n_links, d.n_opt) == (32, 32, n_opt)
    paths = limit_paths(d, T)
    assert paths["rows"] > 128 and paths["par_values"] > 256, paths
    assert paths["parked"] == {"chain": 0, "forked": 3}.get(kind, paths["parked"]) and (kind != "bushy" or paths["parked"] > 4)
    if kind == "chain":
        assert max(np.nonzero(d.parent == np.arange(-1, 31))[0]) == 31  # depth 31
    # forward kinematics of every frame
    q = c.rng.uniform(d.lower, d.upper, size=(16, d.ndof))
    np.testing.assert_allclose(h.eval_fk(q), o.eval_fk(q), rtol=0, atol=1e-12)
    # surface points: offsets and nearest-voxel values bit for bit, and the field's Hessian there
    qs = np.concatenate([c.Q0[0].T[::9], c.qc])
    for use_obs in (False, True):
        xg, og, vg, gg = h.eval_points(0, qs, c.base[0], use_obs=use_obs)
        xo, oo, vo, go = o.eval_points(0, qs, c.base[0], use_obs=use_obs)
        np.testing.assert_allclose(xg, xo, rtol=0, atol=1e-12)
        np.testing.assert_array_equal(og, oo)
        np.testing.assert_array_equal(vg, vo)
        hg = h.eval_points_hessian(0, qs, c.base[0], use_obs=use_obs)
        field = c.scene[1] if use_obs else c.scene[0]
        _, _, ho = oracle_mod.sdf_eval(field, c.scene[2], c.scene[3], c.scene[4], xo.reshape(-1, 3))
        np.testing.assert_array_equal(hg.reshape(-1, 3, 3), ho)
    # objective terms of ragged goal sets, standoff on
    a = h.eval_objective(0, c.goals, c.n_goals, c.S, c.base, c.Q0)
    b = o.eval_objective(0, c.goals, c.n_goals, c.S, c.base, c.Q0)
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_allclose(x, y, rtol=1e-9, atol=1e-13)
    np.testing.assert_array_equal(a[3], b[3])
    # obstacle normal equations
    A, g, ss = h.eval_obstacle_normal_eq(0, c.base, c.Q0)
    Ao, go, sso = o.eval_obstacle_normal_eq(0, c.base, c.Q0)
    assert sso.max() > 0 and (sso[:, 2:] == 0).any(), "the field should reach some waypoints and miss others"
    np.testing.assert_allclose(A[:, 2:], Ao[:, 2:], rtol=1e-8, atol=1e-10 * max(np.abs(Ao).max(), 1e-30))
    np.testing.assert_allclose(g[:, 2:], go[:, 2:], rtol=1e-8, atol=1e-10 * max(np.abs(go).max(), 1e-30))
    np.testing.assert_allclose(ss, sso, rtol=1e-11, atol=1e-15)
    # seed scoring
    cg, dg = h.plan_cost(0, c.Q0, c.base[0])
    co, do = o.plan_cost(0, c.Q0, c.base[0])
    assert co.max() > 0
    np.testing.assert_allclose(cg, co, rtol=1e-12)
    np.testing.assert_allclose(dg, do, rtol=1e-14)
    if n_opt <= 8:  # inverse kinematics and base placement (the IK and base kernels take up to eight optimised joints)
        for sid in (None, 0):
            qi, fi, iti, sti = h.solve_ik_batch(sid, c.qc, c.goals[:, 0], c.base, max_iter=30)
            qo, fo, ito, sto = o.solve_ik_batch(sid, c.qc, c.goals[:, 0], c.base, max_iter=30, n_threads=c.nt)
            np.testing.assert_array_equal(iti, ito)
            np.testing.assert_array_equal(sti, sto)
            np.testing.assert_allclose(qi, qo, rtol=0, atol=1e-6)
            np.testing.assert_allclose(fi, fo, rtol=1e-8, atol=1e-12)
        yg, qg, fg, itg, stg = h.solve_base_batch(c.qc, c.goals, c.n_goals, 0.01, max_iter=25)
        yo, qo, fo, ito, sto = o.solve_base_batch(c.qc, c.goals, c.n_goals, 0.01, max_iter=25, n_threads=c.nt)
        np.testing.assert_array_equal(itg, ito)
        np.testing.assert_array_equal(stg, sto)
        np.testing.assert_allclose(fg, fo, rtol=1e-7, atol=1e-12)
        np.testing.assert_allclose(yg, yo, rtol=0, atol=1e-6)
    c.close()


@pytest.mark.parametrize("T", [50, 96])
@pytest.mark.parametrize("kind,n_opt", ROBOTS)
def test_limit_robot_solve_matches_oracle(capi, oracle_mod, monkeypatch, kind, n_opt, T):
    """The solve of ragged goal sets with the standoff on, against the oracle; then the same call through the launches for
    many instances in flight (GTO_FEW_INSTANCES=0: the step kernel's broad-phase tail on the 8-wide robots that allow it),
    without that broad phase (GTO_PREBROAD=0) and with eight waypoints asked of every obstacle workgroup (GTO_OBS_TG=8,
    more than these robots' LDS holds: gto_create caps it): bit for bit the same trajectories."""
    c = LimitCase(capi, oracle_mod, kind, n_opt, T)
    Qg, dQg, fg, itg, stg = c.h.solve_batch(*c.solve_args())
    Qo, dQo, fo, ito, sto = c.o.solve_batch(*c.solve_args(), n_threads=c.nt)
    np.testing.assert_array_equal(itg, ito)
    np.testing.assert_array_equal(stg, sto)
    assert (itg > 1).all()
    np.testing.assert_allclose(Qg, Qo, rtol=0, atol=1e-6)
    np.testing.assert_allclose(fg, fo, rtol=1e-8)
    c.close()
    ref = None
    for env in ({"GTO_FEW_INSTANCES": "0"}, {"GTO_FEW_INSTANCES": "0", "GTO_PREBROAD": "0"},
                {"GTO_FEW_INSTANCES": "0", "GTO_OBS_TG": "8"}, {"GTO_OBS_TG": "8"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            h = capi.SolverHandle(c.desc, c.ee, c.ee, c.opts, device=0, n_gripper_points=40)
        h.set_scene(0, *c.scene)
        got = h.solve_batch(*c.solve_args())
        h.close()
        if ref is None:
            ref = got
            np.testing.assert_array_equal(ref[3], ito)
            np.testing.assert_allclose(ref[0], Qo, rtol=0, atol=1e-6)
        elif "GTO_FEW_INSTANCES" in env:
            for x, y in zip(ref, got):
                np.testing.assert_array_equal(x, y)
        else:
            for x, y in zip((Qg, dQg, fg, itg, stg), got):
                np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------------------------------ goal sets past one wave
def _panda_goal_batch(capi, oracle_mod, counts, seed=5):
    cfg = cfg_of("panda")
    from grasptrajopt_amd.robot_desc import load_builtin
    d = load_builtin("panda")
    opts = oracle_mod.reference_opts(max_iter=20)
    h = capi.SolverHandle(d, cfg["link_ee"], cfg["link_gripper"], opts, device=0)
    o = oracle_mod.Oracle(d, cfg["link_ee"], cfg["link_gripper"], opts)
    sc = syn.make_scene(2, n=48, res=0.0467, origin=(-0.4, -1.12, -0.4), table_z=-0.03)
    for s in (h, o):
        s.set_scene(0, sc.c_all, sc.c_obs, sc.shape, sc.origin, sc.res)
    B, n_max = len(counts), max(counts)
    RT, qg = syn.make_goals(d, h.eval_fk, cfg["link_ee"], B * n_max, seed=seed, zlim=(0.08, 0.7))
    goals = RT.reshape(B, n_max, 16).copy()
    qc = np.tile(np.array(cfg["default_pose"], dtype=np.float64), (B, 1))
    qg = qg.reshape(B, n_max, d.ndof)
    S = syn.standoff_pose(-0.1, cfg["axis_standoff"])
    base = np.zeros((B, 3))
    return d, cfg, h, o, goals, qc, qg, S, base


def test_goal_sets_larger_than_a_wave_match_oracle(capi, oracle_mod):
    """Ragged sets of 63, 64, 65, 130 and 200 goals.  In each, the goal the seed ends at (the arg-min of the goal term without
    the standoff) is planted at an index of 64 or more where the set has one; a copy of it 64 further on (same lane) and a
    copy at a lower index (another lane) tie with it: optas.mmin picks the lowest index.  A NaN goal past index 64 is never the arg-min and
    changes nothing (the solve is the solve without it: bit for bit the batch where that goal lies far away)."""
    counts = [63, 64, 65, 130, 200, 200, 130]
    d, cfg, h, o, goals, qc, qg, S, base = _panda_goal_batch(capi, oracle_mod, counts)
    B, n_max, T = len(counts), max(counts), 50
    n_goals = np.array(counts, dtype=np.int32)
    fe = d.frame_index(cfg["link_ee"])
    plant = {0: 40, 1: 63, 2: 64, 3: 100, 4: 150, 5: 199, 6: 65}
    Q0 = np.stack([syn.make_seed(qc[b], qg[b, plant[b]], T, d.param_index) for b in range(B)])
    for b, g in plant.items():
        goals[b, g] = o.eval_fk(Q0[b, :, -1][None])[0, fe].reshape(16)
    expect = dict(plant)
    goals[4, 150 - 64] = goals[4, 150]            # lane 22, second and third stride: the tie goes to 86
    expect[4] = 86
    goals[6, 65 + 64] = goals[6, 65]              # lane 1, second and third stride: 65 stays
    goals[3, 100 - 64 + 1] = goals[3, 100]        # lane 37's first stride against lane 36's second: 37
    expect[3] = 37
    # (without the standoff term the planted goal costs nothing at the seed's last waypoint: it and its copies are the minimum)
    a = h.eval_objective(0, goals, n_goals, None, base, Q0)
    b_ = o.eval_objective(0, goals, n_goals, None, base, Q0)
    assert b_[3].tolist() == [expect[b] for b in range(B)], b_[3].tolist()
    np.testing.assert_array_equal(a[3], b_[3])
    np.testing.assert_allclose(a[0], b_[0], rtol=1e-9, atol=1e-14)
    # a NaN goal past index 64 of every set that has one; the clean batch has a far-away goal there instead
    poisoned, far = goals.copy(), goals.copy()
    for b in range(B):
        if counts[b] > 66:
            k = counts[b] - 2 if counts[b] - 2 != plant[b] else counts[b] - 3
            poisoned[b, k, 3] = np.nan
            far[b, k, 3] += 100.0
    ap = h.eval_objective(0, poisoned, n_goals, None, base, Q0)
    np.testing.assert_array_equal(ap[3], a[3])
    np.testing.assert_array_equal(ap[3], o.eval_objective(0, poisoned, n_goals, None, base, Q0)[3])
    a = h.eval_objective(0, poisoned, n_goals, S, base, Q0)  # and with it
    np.testing.assert_array_equal(a[3], o.eval_objective(0, poisoned, n_goals, S, base, Q0)[3])
    ref = h.solve_batch(0, qc, far, n_goals, S, base, Q0)
    got = h.solve_batch(0, qc, poisoned, n_goals, S, base, Q0)
    for x, y in zip(ref, got):
        np.testing.assert_array_equal(x, y)
    Qo, dQo, fo, ito, sto = o.solve_batch(0, qc, poisoned, n_goals, S, base, Q0, n_threads=o.usable_cores())
    np.testing.assert_array_equal(got[3], ito)
    np.testing.assert_array_equal(got[4], sto)
    np.testing.assert_allclose(got[0], Qo, rtol=0, atol=1e-6)
    np.testing.assert_allclose(got[2], fo, rtol=1e-8)
    # the final arg-min of every solved trajectory
    af = h.eval_objective(0, poisoned, n_goals, S, base, got[0])
    np.testing.assert_array_equal(af[3], o.eval_objective(0, poisoned, n_goals, S, base, Qo)[3])
    h.close()


def test_goal_sets_larger_than_a_wave_on_the_wide_limit_robot(capi, oracle_mod):
    """The same first-minimum rule through the 16-wide kernels: 130 goals on chain-16, the arg-min planted at 129 with a
    copy at 65 (one lane, two strides)."""
    c = LimitCase(capi, oracle_mod, "chain", 16, 50, B=3, n_max=130, max_iter=10)
    d, h, o = c.desc, c.h, c.o
    fe = d.frame_index(c.ee)
    c.n_goals[:] = [130, 65, 100]
    c.goals[0, 129] = c.goals[0, 65] = o.eval_fk(c.Q0[0, :, -1][None])[0, fe].reshape(16)
    c.goals[2, 99] = o.eval_fk(c.Q0[2, :, -1][None])[0, fe].reshape(16)
    a = h.eval_objective(0, c.goals, c.n_goals, c.S, c.base, c.Q0)
    b = o.eval_objective(0, c.goals, c.n_goals, c.S, c.base, c.Q0)
    np.testing.assert_array_equal(a[3], b[3])
    assert a[3][0] == 65 and a[3][2] == 99
    Qg, _, fg, itg, stg = h.solve_batch(*c.solve_args())
    Qo, _, fo, ito, sto = o.solve_batch(*c.solve_args(), n_threads=c.nt)
    np.testing.assert_array_equal(itg, ito)
    np.testing.assert_array_equal(stg, sto)
    np.testing.assert_allclose(Qg, Qo, rtol=0, atol=1e-6)
    np.testing.assert_allclose(fg, fo, rtol=1e-8)
    c.close()


def test_plan_goalset_with_100_solutions_matches_oracle(oracle_mod):
    """GTOPlanner.plan_goalset with every one of 100 IK solutions as the goal set, as the driver calls it
    (examples/pybullet_gto_planning.py:291): seed choice, iterations, plan and cost against the oracle path."""
    from test_gpu_planner import _oracle_seed, _setup
    rng = np.random.default_rng(8)
    cfg, robot, planner, orc, c_all, c_obs, RT, qsol = _setup("panda", oracle_mod, 100, rng)
    qc = np.array(cfg["default_pose"])
    base = [0.0, 0.0, 0.0]
    q_solutions = qsol.T.astype(np.float32)
    plan, dQ, cost = planner.plan_goalset(qc, RT, c_all, c_obs, base, q_solutions, use_standoff=True,
                                          axis_standoff=cfg["axis_standoff"], interpolate=True)
    plans, best = _oracle_seed(robot, orc, qc, q_solutions.T.astype(np.float64), c_obs, base)
    assert planner.seed_index == best
    S = syn.standoff_pose(-0.1, cfg["axis_standoff"])
    Qo, dQo, fo, ito, sto = orc.solve_batch(0, qc[None], RT.reshape(1, 100, 16), 100, S, base, plans[best][None])
    assert planner.solver.number_of_iterations() == int(ito[0])
    np.testing.assert_allclose(plan, Qo[0], rtol=0, atol=1e-6)
    np.testing.assert_allclose(cost, fo, rtol=1e-7)
    robot.close()
