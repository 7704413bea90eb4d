"""Solver options away from the reference's constants: the option sets, the problems and the "decided" filter that
tests/test_solver_opts_cpu.py (the oracle against numpy, the cases against their own claims) and
tests/test_gpu_solver_opts.py (the HIP library against the oracle) share.  Imports without a GPU.

Five fields of gto_solver_opts (w_obstacle, w_vel, Tmax, lambda0, tol_step) kept the reference's value in every other GPU
test; every set below moves at least one of them.  The shapes are the smallest that still reach every code path: T = 8 with
the standoff at waypoint 5, six instances, a 32^3 field over the workspace of helpers.Problem (2.24 m a side).
"""
import numpy as np

import ik_pose_cases as ipc
import ik_pose_ref as ipr
import retrieve_ref as rr
from grasptrajopt_amd import synthetic as syn
from grasptrajopt_amd.robot_desc import load_builtin
from helpers import Problem, cfg_of

T, OFFSET, B = 8, -3, 6
CAP = 40          # iteration cap of the sets that do not name one (some instances run into it: status 1 is compared too)
SMALL_CAP = 6     # runs_to_cap
EPS = 1e-13       # the decided filter's move of a seed
Q_STABLE = 1e-9   # ... and what the oracle's own answer may change by under it

OPTION_SETS = {
    "reference": {},                                       # the control
    "obstacle_heavy": dict(w_obstacle=250.0),              # 25 x
    "obstacle_off": dict(w_obstacle=0.0),                  # the facade's value without an obstacle term
    "velocity_stiff": dict(w_vel=1.0),                     # 100 x
    "velocity_off": dict(w_vel=0.0),                       # alpha = 0: the block-tridiagonal system falls apart into blocks
    "time_short": dict(Tmax=0.5),                          # alpha 400 x
    "time_long": dict(Tmax=200.0),                         # alpha / 400
    "damping_small": dict(lambda0=1e-6),                   # the first rounds reject, or accept tiny steps
    "damping_large": dict(lambda0=10.0),
    "ends_by_step": dict(tol_rel_f=0.0, tol_step=3e-3),    # the step-tolerance test is what ends the solve
    "runs_to_cap": dict(tol_rel_f=0.0, tol_step=0.0, max_iter=SMALL_CAP),  # neither tolerance can fire
    "mixed": dict(w_obstacle=3.7, w_vel=0.045, Tmax=3.1, lambda0=0.02, tol_step=1e-5),  # all five at once
}
NAMES = list(OPTION_SETS)
LOSE_NONE = ("reference", "runs_to_cap")


def opts_of(oracle_mod, name, **kw):
    """gto_solver_opts of a named set at this file's horizon; kw overrides (max_iter for the capped comparisons)."""
    o = dict(T=T, standoff_offset=OFFSET, max_iter=CAP)
    o.update(OPTION_SETS[name])
    o.update(kw)
    return oracle_mod.reference_opts(**o)


def cap_of(name, default=CAP):
    return OPTION_SETS[name].get("max_iter", default)


# ---------------------------------------------------------------------------------------------------------------- problems
# (robot, goals per set, standoff, scene seed, picks): panda and fetch for the narrow step kernel, fetch_mobile (ten
# optimised joints) for the wide one; one-goal and three-goal sets, with and without a standoff.  Each problem is drawn as
# a pool of 16 instances, and `picks` names the six that are solved: chosen on the CPU so that the oracle alone is decided
# on every one of them under every option set, capped solves included (test_solver_opts_cpu asserts it), that
# `ends_by_step` converges on each, and with as many other endings below the cap as the pool offers.
TRAJ = {
    "panda_1_standoff": ("panda", 1, True, 3, (2, 4, 5, 10, 12, 15)),
    "panda_3_plain": ("panda", 3, False, 2, (1, 4, 6, 9, 10, 15)),
    "fetch_3_standoff": ("fetch", 3, True, 1, (4, 5, 8, 10, 12, 13)),
    "fetch_1_plain": ("fetch", 1, False, 4, (2, 5, 9, 12, 14, 15)),
    "wide_1_standoff": ("fetch_mobile", 1, True, 5, (0, 3, 6, 7, 10, 12)),
    "wide_3_plain": ("fetch_mobile", 3, False, 5, (0, 2, 10, 11, 13, 14)),
}
POOL = 16
NARROW = [k for k in TRAJ if not k.startswith("wide")]
N_FIELD, RES_FIELD = 32, 0.07

_CACHE = {}


def traj_problem(oracle_mod, key):
    """helpers.Problem of TRAJ[key], finished with the ORACLE's forward kinematics (the CPU file vets exactly these
    numbers; the GPU file then hands the same ones to both sides)."""
    if ("traj", key) not in _CACHE:
        robot, n_goals, standoff, seed, picks = TRAJ[key]
        p = Problem(robot, B=POOL, scene_seed=seed, n=N_FIELD, res=RES_FIELD, n_goals=n_goals, T=T, use_standoff=standoff)
        o = oracle_mod.Oracle(p.desc, p.cfg["link_ee"], p.cfg["link_gripper"], oracle_mod.reference_opts(T=T, standoff_offset=OFFSET))
        p.finish(o.eval_fk)
        picks = list(picks)
        p.B = len(picks)
        p.qc, p.base, p.goals, p.qgoal, p.Q0 = p.qc[picks], p.base[picks], p.goals[picks], p.qgoal[picks], p.Q0[picks]
        # a trajectory off the seed for the objective comparison (as test_objective_terms_vs_oracle builds its)
        rng = np.random.default_rng(11)
        oi = p.desc.opt_index
        p.Q_eval = p.Q0.copy()
        p.Q_eval[:, oi, 2:] += 0.05 * rng.standard_normal(p.Q_eval[:, oi, 2:].shape)
        _CACHE["traj", key] = p
    return _CACHE["traj", key]


DENSE = 1  # scene id of the dense field


def dense_scene_args(prob, sid=DENSE):
    """A dense random field on the problem's grid (as test_obstacle_normal_equations_vs_oracle builds its): every surface
    point of every robot carries a cost value at every waypoint, so f_obs is far from zero whatever the trajectory (the
    synthetic scene leaves the fetch's seeds untouched: its f_obs there is an exact 0, which scales to anything)."""
    sc = prob.scene
    rng = np.random.default_rng(5)
    ca = (0.05 * rng.random(sc.c_all.size)).astype(np.float32)
    co = (0.05 * rng.random(sc.c_all.size)).astype(np.float32)
    return (sid, ca, co, sc.shape, sc.origin, sc.res)


def oracle_for(oracle_mod, prob, opts, scene=True):
    """The oracle of a problem: scene 0 the problem's synthetic scene (the solves), scene DENSE the dense field (the terms)."""
    o = oracle_mod.Oracle(prob.desc, prob.cfg["link_ee"], prob.cfg["link_gripper"], opts)
    if scene:
        o.set_scene(*prob.scene_args())
        o.set_scene(*dense_scene_args(prob))
    return o


def moved(prob, eps):
    """solve_args with the seeds' optimised entries (the free waypoints) moved by eps."""
    a = list(prob.solve_args())
    Q0 = a[6].copy()
    Q0[:, prob.desc.opt_index, 2:] += eps
    a[6] = Q0
    return tuple(a)


def _stable(base, others):
    """Per instance: the same iterations and status, and the answer within Q_STABLE, in every run of `others`."""
    Q, it, st = base
    ok = np.ones(len(it), dtype=bool)
    for Q2, it2, st2 in others:
        d = np.abs(np.asarray(Q2) - Q).reshape(len(it), -1).max(axis=1)
        ok &= (it2 == it) & (st2 == st) & (d <= Q_STABLE)
    return ok


def traj_oracle(oracle_mod, key, name, **kw):
    """(Q, dQ, f, iters, status) of the oracle on TRAJ[key] under set `name`; cached."""
    ck = ("sol", key, name, tuple(sorted(kw.items())))
    if ck not in _CACHE:
        p = traj_problem(oracle_mod, key)
        _CACHE[ck] = oracle_for(oracle_mod, p, opts_of(oracle_mod, name, **kw)).solve_batch(*p.solve_args())
    return _CACHE[ck]


def traj_decided(oracle_mod, key, name, **kw):
    """Boolean (B,): the instances on which the oracle alone is decided (see the module docstring of the CPU test)."""
    ck = ("dec", key, name, tuple(sorted(kw.items())))
    if ck not in _CACHE:
        p = traj_problem(oracle_mod, key)
        o = oracle_for(oracle_mod, p, opts_of(oracle_mod, name, **kw))
        Q, _, _, it, st = traj_oracle(oracle_mod, key, name, **kw)
        runs = []
        for e in (EPS, -EPS):
            Q2, _, _, it2, st2 = o.solve_batch(*moved(p, e))
            runs.append((Q2, it2, st2))
        _CACHE[ck] = _stable((Q, it, st), runs)
    return _CACHE[ck]


def within_cap(name, decided):
    """The filter's cap: at most one instance in eight left out; none on the control and on runs_to_cap."""
    out = int((~decided).sum())
    return out == 0 if name in LOSE_NONE else out * 8 <= len(decided)


# ------------------------------------------------------------------------------------------- numpy restatement of the terms
def independent_terms(o, prob, opts, Q, sid=0):
    """f_goal, f_obs, f_vel, arg-min of gto/gto_planner.py:84-135 in numpy, from the options and from eval_fk / eval_points
    alone (pinned against the reference's fixtures elsewhere): none of the oracle's objective code is used.
      f_goal  min over the goals of the gripper points' squared distances at the last waypoint (+ at the standoff waypoint
              T + standoff_offset to RT @ S);
      f_obs   w_obstacle * sum of squared cost values, sdf_cost_all before the standoff waypoint, sdf_cost_obstacle from it on;
      f_vel   w_vel * sum of squared velocities, dQ_t = (Q_{t+1} - Q_t) / dt, dt = Tmax / (T - 1), dQ_0 = 0."""
    d = prob.desc
    Tn, ts = int(opts.T), int(opts.T + opts.standoff_offset)
    dt = opts.Tmax / (Tn - 1)
    oi = d.opt_index
    Bn = Q.shape[0]
    fe, fg_ = d.frame_index(prob.cfg["link_ee"]), d.frame_index(prob.cfg["link_gripper"])
    gp = d.link_points(prob.cfg["link_gripper"])
    gph = np.concatenate([gp, np.ones((len(gp), 1))], axis=1)
    f_goal, f_obs, f_vel, am = np.empty(Bn), np.empty(Bn), np.empty(Bn), np.empty(Bn, dtype=np.int32)
    for b in range(Bn):
        ss = 0.0
        for t in range(Tn):
            val = o.eval_points(sid, Q[b, :, t][None], prob.base[b], use_obs=(t >= ts))[2]
            ss += float((val[0] ** 2).sum())
        f_obs[b] = opts.w_obstacle * ss
        v = (Q[b, oi, 2:] - Q[b, oi, 1:-1]) / dt
        f_vel[b] = opts.w_vel * float((v ** 2).sum())
        cost = np.zeros(prob.n_goals)
        for t, S in ((Tn - 1, None),) + (((ts, prob.S),) if prob.S is not None else ()):
            fr = o.eval_fk(Q[b, :, t][None])[0]
            G = np.linalg.inv(fr[fe]) @ fr[fg_]
            xa = gph @ fr[fg_].T
            for g in range(prob.n_goals):
                RT = prob.goals[b, g].reshape(4, 4)
                Y = (RT if S is None else RT @ np.asarray(S).reshape(4, 4)) @ G
                cost[g] += float(((xa - gph @ Y.T)[:, :3] ** 2).sum())
        am[b] = int(np.argmin(cost))
        f_goal[b] = cost[am[b]]
    return f_goal, f_obs, f_vel, am


# ---------------------------------------------------------------------------------------------------------- the other solvers
IK_B, IK_POOL = 8, 16
# instances of the pool of 16 on which the oracle alone is decided under every option set, with and without the scene: four
# with the far seed (the default pose), four with a seed near the goal's configuration
IK_PICKS = {"panda": (0, 2, 3, 4, 8, 9, 10, 11), "fetch": (0, 2, 3, 5, 8, 9, 10, 11)}
IK_ROBOTS = tuple(IK_PICKS)


def ik_problem(oracle_mod, robot):
    """(prob, q0): eight goals, half of the seeds far (the default pose) and half near (as test_ik_matches_oracle builds them)."""
    if ("ik", robot) not in _CACHE:
        p = Problem(robot, B=IK_POOL, scene_seed=5, n=N_FIELD, res=RES_FIELD, T=T)
        o = oracle_mod.Oracle(p.desc, p.cfg["link_ee"], p.cfg["link_gripper"], oracle_mod.reference_opts(T=T, standoff_offset=OFFSET))
        p.finish(o.eval_fk)
        rng = np.random.default_rng(1)
        q0 = np.tile(np.array(p.cfg["default_pose"], dtype=np.float64), (IK_POOL, 1))
        oi = p.desc.opt_index
        q0[IK_POOL // 2:, oi] = p.qgoal[IK_POOL // 2:, 0][:, oi] + rng.uniform(-0.3, 0.3, size=(IK_POOL // 2, len(oi)))
        picks = list(IK_PICKS[robot])
        p.B, q0 = len(picks), q0[picks]
        p.qc, p.base, p.goals, p.qgoal, p.Q0 = p.qc[picks], p.base[picks], p.goals[picks], p.qgoal[picks], p.Q0[picks]
        _CACHE["ik", robot] = (p, q0)
    return _CACHE["ik", robot]


def ik_oracle(oracle_mod, robot, name, collide):
    """((q, f, iters, status), decided) of the oracle's IK under set `name`; the cap is the set's own, or the reference's 50."""
    ck = ("iksol", robot, name, collide)
    if ck not in _CACHE:
        p, q0 = ik_problem(oracle_mod, robot)
        o = oracle_for(oracle_mod, p, opts_of(oracle_mod, name))
        sid, cap, oi = (0 if collide else None), cap_of(name, 50), p.desc.opt_index
        run = lambda q: o.solve_ik_batch(sid, q, p.goals[:, 0], p.base, max_iter=cap)
        res = run(q0)
        runs = []
        for e in (EPS, -EPS):
            q = q0.copy()
            q[:, oi] += e
            r = run(q)
            runs.append((r[0], r[2], r[3]))
        _CACHE[ck] = (res, _stable((res[0], res[2], res[3]), runs))
    return _CACHE[ck]


# A firm effort weight (the one tests/independent.py uses): with the reference's 0.01 the arm absorbs base motion along a
# nearly flat valley, and at lambda0 = 1e-6 the oracle's own first step then turns a 1e-13 move of the seed into 5e-10 to
# 6e-9 rad (measured) -- undecided by the filter below before any kernel is asked.  At 1.0 it stays below 1e-9 everywhere.
BASE_B, BASE_N, BASE_W, BASE_CAP = 3, 4, 1.0, 25
BASE_POOL, BASE_PICKS = 8, (0, 2, 3)  # the goal sets of the pool (4, 3 and 1 goals) on which the oracle alone is decided under every set


def base_problem(oracle_mod, robot="fetch"):
    if ("base", robot) not in _CACHE:
        cfg, desc = cfg_of(robot), load_builtin(robot)
        o = oracle_mod.Oracle(desc, cfg["link_ee"], cfg["link_gripper"], oracle_mod.reference_opts(), n_gripper_points=100)
        qc = np.array(cfg["default_pose"], dtype=np.float64)
        goals, _ = syn.make_base_goal_sets(desc, o.eval_fk, cfg["link_ee"], qc, BASE_POOL, BASE_N, seed=3)
        QC = np.tile(qc, (BASE_POOL, 1))
        QC[1:, desc.opt_index] += np.random.default_rng(2).uniform(-0.1, 0.1, size=(BASE_POOL - 1, len(desc.opt_index)))
        ng = np.array([4, 2, 3, 1, 4, 2, 3, 4], dtype=np.int32)  # ragged
        picks = list(BASE_PICKS)
        QC, goals, ng = QC[picks], np.ascontiguousarray(goals[picks]), ng[picks]
        _CACHE["base", robot] = (desc, cfg, QC, goals, ng)
    return _CACHE["base", robot]


def base_oracle(oracle_mod, name, robot="fetch"):
    """((y, q, f, iters, status), decided) of the oracle's base placement under set `name`."""
    ck = ("basesol", robot, name)
    if ck not in _CACHE:
        desc, cfg, QC, goals, ng = base_problem(oracle_mod, robot)
        o = oracle_mod.Oracle(desc, cfg["link_ee"], cfg["link_gripper"], opts_of(oracle_mod, name), n_gripper_points=100)
        cap = cap_of(name, BASE_CAP)
        run = lambda qc: o.solve_base_batch(qc, goals, ng, effort_weight=BASE_W, max_iter=cap)
        res = run(QC)
        pack = lambda r: (np.concatenate([r[0], r[1].reshape(BASE_B, -1)], axis=1), r[3], r[4])
        runs = []
        for e in (EPS, -EPS):
            qc = QC.copy()
            qc[:, desc.opt_index] += e
            runs.append(pack(run(qc)))
        _CACHE[ck] = (res, _stable(pack(res), runs))
    return _CACHE[ck]


LIFT_K, LIFT_B = 3, 3


def lift_problem(oracle_mod, robot, collide):
    """(desc, cfg, plans (3, ndof, T), scene or None): the retrieve lift of tests/test_gpu_retrieve.py at this file's horizon."""
    if ("lift", robot, collide) not in _CACHE:
        if collide:
            desc0, cfg0 = load_builtin(robot), cfg_of(robot)
            o = oracle_mod.Oracle(desc0, cfg0["link_ee"], cfg0["link_gripper"], oracle_mod.reference_opts())
            desc, cfg, plans, scene = rr.board_case(robot, o.eval_fk)
            plans = np.ascontiguousarray(plans[:, :, -T:])  # (the lift reads a plan's last column)
        else:
            desc, cfg, plans = rr.grasp_plans(robot, LIFT_B, T=T)
            scene = None
        _CACHE["lift", robot, collide] = (desc, cfg, plans, scene)
    return _CACHE["lift", robot, collide]


def lift_oracle(oracle_mod, robot, name, collide):
    """(chain dict of retrieve_ref.lift_chain on the oracle, decided (B,))."""
    ck = ("liftsol", robot, name, collide)
    if ck not in _CACHE:
        desc, cfg, plans, scene = lift_problem(oracle_mod, robot, collide)
        o = oracle_mod.Oracle(desc, cfg["link_ee"], cfg["link_gripper"], opts_of(oracle_mod, name))
        sid = base = None
        if collide:
            o.set_scene(0, *scene)
            sid, base = 0, np.zeros((len(plans), 3))
        closed, cap = rr.finger_joints(desc), cap_of(name, rr.MAX_ITER)
        run = lambda pl: rr.lift_chain(o, desc, cfg["link_ee"], pl, rr.LIFT[robot] * LIFT_K / 10, LIFT_K, closed_joints=closed,
                                       scene_id=sid, base_pos=base, max_iter=cap)
        res = run(plans)
        pack = lambda r: (r["path"], r["iters"].sum(axis=1) * 1000 + r["iters"].max(axis=1), (r["status"] * 4 ** np.arange(LIFT_K)).sum(axis=1))
        runs = []
        for e in (EPS, -EPS):
            pl = plans.copy()
            pl[:, desc.opt_index, -1] += e
            runs.append(pack(run(pl)))
        _CACHE[ck] = (res, _stable(pack(res), runs))
    return _CACHE[ck]


# pose goals (quaternion and roll-pitch-yaw): cases of tests/ik_pose_cases.py away from every branch boundary, against the
# numpy restatement tests/ik_pose_ref.py, which takes the options
POSE_PER_KIND = 4


def pose_cases():
    if "pose" not in _CACHE:
        q = [c for c in ipc._quaternion_cases() if c.name in ("q_w0", "q_w1", "q_x0", "q_z1")]
        r = [c for c in ipc._rpy_cases() if c.cls == "graded" and c.d >= 1e-2][:POSE_PER_KIND]
        assert len(q) == POSE_PER_KIND and len(r) == POSE_PER_KIND
        _CACHE["pose"] = (ipc.gimbal_robot(), q + r)
    return _CACHE["pose"]


def pose_oracle(oracle_mod, name):
    """([(q, f, iters, status) per case], decided) of the restatement under set `name` (no collision term)."""
    ck = ("posesol", name)
    if ck not in _CACHE:
        desc, cases = pose_cases()
        opts = opts_of(oracle_mod, name)
        o = oracle_mod.Oracle(desc, ipc.EE, ipc.EE, opts)
        cap = cap_of(name, 50)
        res, dec = [], []
        for c in cases:
            p = ipc.problem(o, desc, c)
            r = ipr.solve(p, c.q0, opts, cap)
            ok = True
            for e in (EPS, -EPS):
                q0 = np.array(c.q0, dtype=np.float64)
                q0[desc.opt_index] += e
                r2 = ipr.solve(p, q0, opts, cap)
                ok &= r2[2:] == r[2:] and np.abs(r2[0] - r[0]).max() <= Q_STABLE
            res.append(r)
            dec.append(ok)
        _CACHE[ck] = (res, np.array(dec))
    return _CACHE[ck]
