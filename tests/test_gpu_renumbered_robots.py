"""GPU: every joint-indexed entry point on robots with renumbered joints (tests/renumbered_robots.py: two random trees with
parameter joints between the optimised ones, one with 13 parameter joints, Panda with the fingers first and the arm reversed,
a 10-joint tree for the 16-wide kernels; each in a chain-order variant, where only the joints' numbers change, and a sorted
variant, where the optimised slots change their order too).  Renumbering the joints gives the same robot: an output that sums
nothing over joints or slots must be the original robot's output with its joint axes permuted, bit for bit, in both variants;
so must every output in the chain-order variant; the sorted variant's solves and sums over slots are held to the FP64 oracle
(oracle/gto_oracle.c) and the numpy restatements on the renumbered robot with equal iteration counts and statuses, at the
tolerances the suites of the same entry points state (quoted beside each use).  tests/test_renumbered_robots_cpu.py shows on
the CPU that the oracle's own results are invariant, so no case is set aside.  No call has more than 8 instances.  Run the
file under a time limit and stop at the first fault: timeout -k 10 600 pytest -x tests/test_gpu_renumbered_robots.py."""
import numpy as np
import pytest

import base_chain_ref as bref
import cloud_cases as cc
import depth_cases as dc
import grasp_chain_ref as gref
import ik_pose_ref as pref
import multistart_ref as mref
import renumbered_robots as rn
import retrieve_ref as rr
import small_robots as sr

pytestmark = pytest.mark.gpu

ALL = list(rn.CASES)
NARROW = list(rn.NARROW)
OK = (0, 1)  # GTO_STATUS_CONVERGED, GTO_STATUS_MAX_ITER
WORST = {}   # entry point -> largest difference from the oracle / restatement seen on the renumbered robots (printed)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def rigs(capi, oracle_mod):
    """case name -> {"original", "chain", "sorted"} -> the view with its handle (.h), its oracle (.o) and .nt."""
    made = {}

    def get(name):
        if name not in made:
            c = rn.Case(oracle_mod, name)
            made[name] = {}
            for variant in ("original",) + rn.VARIANTS:
                v = c.view(variant)
                v.h, v.o = v.handle(capi), v.oracle(oracle_mod)
                v.nt = v.o.usable_cores()
                made[name][variant] = v
        return made[name]
    yield get
    for name, views in made.items():
        for v in views.values():
            v.h.close()
    for k, x in sorted(WORST.items()):
        print(f"largest difference from the oracle on the renumbered robots: {k}: {x:.3e}")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def worst(key, got, want, relative=False):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return
    d = np.abs(got - want)
    if relative:
        d = d / np.maximum(np.abs(want), 1e-300)
    d = d[np.isfinite(d)]
    if d.size:
        WORST[key] = max(WORST.get(key, 0.0), float(d.max()))


def cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def renumbered(views):
    return [views[v] for v in rn.VARIANTS]


# =================================================================================================== A. nothing summed over joints
@pytest.mark.parametrize("name", ALL)
def test_kinematics_and_points(rigs, oracle_mod, name):
    """A1: gto_eval_fk, gto_eval_points (xyz, offsets, values, gradient), gto_eval_points_hessian."""
    views = rigs(name)
    v0 = views["original"]
    q = np.random.default_rng(3).uniform(v0.desc.lower, v0.desc.upper, size=(6, v0.desc.ndof))
    fk0 = v0.h.eval_fk(q)
    pts0 = {u: v0.h.eval_points(0, v0.qc, v0.base[0], use_obs=u) for u in (False, True)}
    hes0 = {u: v0.h.eval_points_hessian(0, v0.qc, v0.base[0], use_obs=u) for u in (False, True)}
    for v in renumbered(views):
        fk = v.h.eval_fk(v.new(q, 1))
        assert same(fk, fk0), v.variant
        fko = v.o.eval_fk(v.new(q, 1))
        worst("eval_fk", fk, fko)
        np.testing.assert_allclose(fk, fko, rtol=0, atol=1e-12)     # tests/test_gpu_parity.py:550
        for u in (False, True):
            got = v.h.eval_points(0, v.qc, v.base[0], use_obs=u)
            for x, y in zip(got, pts0[u]):
                assert same(x, y), (v.variant, u)
            xo, oo, vo, go = v.o.eval_points(0, v.qc, v.base[0], use_obs=u)
            worst("eval_points xyz", got[0], xo)
            worst("eval_points gradient", got[3], go)
            np.testing.assert_allclose(got[0], xo, rtol=0, atol=1e-12)  # tests/test_gpu_parity.py:6 (FK / points / gradients)
            np.testing.assert_array_equal(got[1], oo)
            np.testing.assert_array_equal(got[2], vo)
            np.testing.assert_allclose(got[3], go, rtol=0, atol=1e-12)
            hg = v.h.eval_points_hessian(0, v.qc, v.base[0], use_obs=u)
            assert same(hg, hes0[u]), (v.variant, u)
            fld = v.scene[1] if u else v.scene[0]
            _, _, ho = oracle_mod.sdf_eval(fld, v.scene[2], v.scene[3], v.scene[4], xo.reshape(-1, 3))
            np.testing.assert_array_equal(hg.reshape(-1, 3, 3), ho)  # tests/test_gpu_small_robots.py:72
    assert (pts0[True][2] > 0).any() and (pts0[False][2] > 0).any()     # both fields are met


@pytest.mark.parametrize("name", ALL)
def test_plan_cost(rigs, name):
    """A2: gto_plan_cost."""
    views = rigs(name)
    v0 = views["original"]
    c0, d0 = v0.h.plan_cost(0, v0.Q0, v0.base[1])
    assert (c0 > 0).any()
    for v in renumbered(views):
        c, d = v.h.plan_cost(0, v.Q0, v.base[1])
        assert same(c, c0), v.variant
        co, do = v.o.plan_cost(0, v.Q0, v.base[1])
        worst("plan_cost cost (relative)", c, co, True)
        worst("plan_cost distance (relative)", d, do, True)
        np.testing.assert_allclose(c, co, rtol=1e-12)           # tests/test_gpu_parity.py:166
        # the distance |q_0 - q_{T-1}| is a sum of squares over the actuated joints in joint order (gto_plan_cost's host
        # loop over j < ndof, as orc_plan_cost): renumbering reorders it in both variants, so it is not compared bit for bit
        # with the original's but held to the oracle on the renumbered robot, and to the original's value, at
        # tests/test_gpu_parity.py:167
        np.testing.assert_allclose(d, do, rtol=1e-14)
        np.testing.assert_allclose(d, d0, rtol=1e-14)


def _observed(v0, kind, T):
    """An observation and B = 3 plans of T columns in the original numbering with the oracle's counts (shared base and
    per-plan bases), by depth_cases.plan_instance / cloud_cases.plan_cloud on the original robot."""
    from grasptrajopt_amd.observation import Observation
    inst, poisoned, want, n_undecided = rn.plan_inputs(v0, v0.o, kind, T)
    assert n_undecided == 0, (kind, T)
    if kind == "depth":
        obs = Observation.from_depth(inst.depth, inst.K, inst.cam, None, inst.threshold)
    else:
        obs = Observation.from_cloud(inst.points, inst.normals, cc.PLAN_K)
    return inst, obs, poisoned, want


@pytest.mark.parametrize("kind", ["depth", "cloud"])
@pytest.mark.parametrize("name", ALL)
def test_check_plans_and_check_paths(rigs, name, kind):
    """A3: gto_check_plans, and gto_check_paths on 65 columns (the path of a 64-step lift; more than the handle's T)."""
    views = rigs(name)
    v0 = views["original"]
    for T, call in ((v0.T, "check_plans"), (rn.PATH_COLUMNS, "check_paths")):
        assert call == "check_plans" or T > v0.h.T
        inst, obs, poisoned, want = _observed(v0, kind, T)
        p, _, t = inst.nan_at
        for label, bases in (("shared", inst.base), ("per_plan", inst.bases)):
            assert want[label][p, t] == -1 and (want[label] > 0).any() and (want[label] == 0).any()
            g0 = getattr(v0.h, call)(obs, poisoned, bases)
            assert g0.shape == (dc.PLAN_B, T)
            np.testing.assert_array_equal(g0, want[label])
            for v in renumbered(views):
                g = getattr(v.h, call)(obs, v.new(poisoned, 1), bases)
                np.testing.assert_array_equal(g, want[label], err_msg=f"{v.variant} {label}")
        obs.close()


def _ik_report(v, sid, q, RT, base, tols):
    import torch
    from test_gpu_grasp_chain import dev_empty
    B = len(q)
    outs = [dev_empty((B,), torch.float64) for _ in range(3)] + [dev_empty((B,), torch.uint8, 9)]
    keep = [cu(sid), cu(q), cu(RT.reshape(B, 16)), cu(base)]
    torch.cuda.synchronize()
    v.h.ik_report_device(B, *[x.data_ptr() for x in keep], *tols, *[x.data_ptr() for x in outs])
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in outs]


@pytest.mark.parametrize("name", NARROW)
def test_ik_report(rigs, name):
    """A4: gto_ik_report_device as tests/test_gpu_seed_waves.py::test_report_on_other_robots_against_the_oracle holds it."""
    from test_gpu_grasp_chain import widest_gap
    views = rigs(name)
    v0 = views["original"]
    d, o, B = v0.desc, v0.o, 8
    fe = d.frame_index(v0.ee)
    rng = np.random.default_rng(31 + v0.T)
    q = rng.uniform(d.lower, d.upper, (B, d.ndof))
    base = rng.uniform(-0.03, 0.03, (B, 3))
    off = rng.uniform(-1.0, 1.0, (B, d.ndof)) * np.linspace(0.0, 0.3, B)[:, None] * (d.upper - d.lower)[None, :]
    tf_o = o.eval_fk(q)[:, fe]
    RT = o.eval_fk(np.clip(q + off, d.lower, d.upper))[:, fe]
    cost_o = np.stack([o.eval_points(0, q[b:b + 1], base[b], use_obs=True)[2].sum(axis=1)[0] for b in range(B)])
    ep_o, er_o, _ = gref.report(tf_o, RT, cost_o, 1.0, 1.0, 1.0)
    pos_tol, m_pos = widest_gap(ep_o, 1e-3)
    rot_tol, m_rot = widest_gap(er_o, 1e-2)
    cost_tol, m_cost = widest_gap(cost_o, 1.0)
    assert m_pos > 1e-9 and m_rot > 1e-3 and m_cost > 1e-9 * max(1.0, np.abs(cost_o).max())
    acc = gref.report(tf_o, RT, cost_o, pos_tol, rot_tol, cost_tol)[2]
    sid = np.zeros(B, np.int32)
    g0 = _ik_report(v0, sid, q, RT, base, (pos_tol, rot_tol, cost_tol))
    for v in renumbered(views):
        g = _ik_report(v, sid, v.new(q, 1), RT, base, (pos_tol, rot_tol, cost_tol))
        for x, y in zip(g, g0):
            assert same(x, y), v.variant
        worst("ik_report err_pos", g[0], ep_o)
        worst("ik_report err_rot (degrees)", g[1], er_o)
        worst("ik_report cost (relative)", g[2], cost_o, True)
        np.testing.assert_allclose(g[0], ep_o, rtol=0, atol=1e-12)   # tests/test_gpu_seed_waves.py:333-336
        np.testing.assert_allclose(g[1], er_o, rtol=0, atol=1e-5)
        np.testing.assert_allclose(g[2], cost_o, rtol=1e-11, atol=0)
        assert np.array_equal(g[3].astype(bool), acc)


@pytest.mark.parametrize("name", NARROW)
def test_retrieve_reverse(rigs, name):
    """A5: gto_retrieve_reverse_device with closed parameter joints at distinct non-zero values."""
    import torch
    views = rigs(name)
    v0 = views["original"]
    B = 5
    plans0 = np.random.default_rng(v0.T).standard_normal((B, v0.desc.ndof, v0.T))
    want0 = rr.reverse_path(plans0, rn.OFFSET, v0.closed_joints, v0.closed_values)
    assert (want0[:, v0.closed_joints, :] == np.asarray(v0.closed_values)[None, :, None]).all()
    for v in [v0] + renumbered(views):
        n = v.h.retrieve_path_columns()
        assert n == 9 - rn.OFFSET
        plans = v.new(plans0, 1)
        d_plans, d_path = cu(plans), torch.full((B, v.desc.ndof, n), -7.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        assert v.h.retrieve_reverse(B, d_plans.data_ptr(), v.closed_joints, v.closed_values, d_path.data_ptr()) == n
        torch.cuda.synchronize()
        got = d_path.cpu().numpy()
        assert same(got, rr.reverse_path(plans, rn.OFFSET, v.closed_joints, v.closed_values)), v.variant
        assert same(v.old(got, 1), want0), v.variant


@pytest.mark.parametrize("name", NARROW)
def test_retime(rigs, name):
    """A6: gto_retime_batch with vmax / amax permuted, two joints standing still in two plans, every third joint without a
    velocity limit.  The pass kernel takes minima over the joints' lines, so the joints' order does not reach the bits."""
    from test_gpu_retime import KEYS, _check_against_ref
    views = rigs(name)
    v0 = views["original"]
    plans0, vm0, am0 = rn.retime_inputs(v0)
    assert np.isinf(vm0).any() and np.isfinite(vm0).any()
    g0 = _check_against_ref(v0.desc, v0.h, plans0, subdiv=2, M=16, vmax=vm0, amax=am0)
    assert (g0["status"] == 0).all()
    for v in renumbered(views):
        plans, vm, am = rn.retime_inputs(v)
        g = _check_against_ref(v.desc, v.h, plans, subdiv=2, M=16, vmax=vm, amax=am)
        for k in KEYS + ("status",):
            x = v.old(g[k], 2) if k in ("q", "qd", "qdd") else g[k]
            assert same(x, g0[k]), (v.variant, k)


def _dynamics(v):
    q, qd, qdd, pl = rn.dynamics_inputs(v)
    return v.h.inverse_dynamics(q, qd, qdd, dict(mass=pl[0], com=pl[1], inertia=pl[2]))


@pytest.mark.parametrize("name", ALL)
def test_inverse_dynamics(rigs, name):
    """A7: gto_inverse_dynamics over 20 rows with a payload (mass, centre of mass, inertia) on the end effector.  rt_rnea
    (csrc/gto_dynamics.h) walks the FRAMES; a joint's number only addresses the loads of q, qd, qdd and the store of tau, and
    opt_index is not read: the torques are the original robot's, permuted, bit for bit in both variants, and the variants
    give each other's bits.  The original is held to tests/dynamics_ref.py at the 1e-11 of tests/test_gpu_dynamics.py
    (tests/test_renumbered_robots_cpu.py: the yardstick itself is invariant bit for bit)."""
    import dynamics_ref as dr
    views = rigs(name)
    v0 = views["original"]
    q, qd, qdd, pl = rn.dynamics_inputs(v0)
    tau0 = _dynamics(v0)
    ref = dr.inverse_dynamics_rows(v0.desc, q, qd, qdd, v0.desc.frame_index(v0.ee), pl)
    err = np.abs(tau0 - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))
    print(f"{name}: inverse dynamics, max relative error {err.max():.3e}, |tau|_inf {np.abs(ref).max():.3f}")
    WORST["inverse_dynamics (relative to max(1, |tau|_inf))"] = max(WORST.get("inverse_dynamics (relative to max(1, |tau|_inf))", 0.0), float(err.max()))
    assert tau0.shape == ref.shape and np.isfinite(tau0).all() and err.max() <= 1e-11
    assert np.abs(ref - dr.inverse_dynamics_rows(v0.desc, q, qd, qdd)).max() > 1e-3   # the payload is felt
    got = {v.variant: _dynamics(v) for v in renumbered(views)}
    for v in renumbered(views):
        assert not same(got[v.variant], tau0) and same(v.old(got[v.variant], 1), tau0), v.variant
    assert same(got["chain"], got["sorted"])   # the same q_index; opt_index is not read


RETIME_CONVEX_GAP = 1e-8


@pytest.mark.parametrize("name", NARROW + ["r55"])
def test_retime_convex(rigs, name):
    """A8: gto_retime_paths_convex on the inputs of A6, subdiv = 2, M = 16, gap_tol = 1e-8.  Per view: the restatement
    (tests/retime_convex_ref.py on the view's own paths and limits), feasibility and the greedy call, by
    tests/test_gpu_retime_convex._against_reference_and_greedy.  Across views: k_retime_convex sums barrier terms over the
    joints, so a renumbered view takes other Newton steps to another point of the same certified interval: statuses are
    equal, and both durations lie in [T*, (1 + gap_tol) T*], so |d_v - d_0| <= gap_tol min(d_v, d_0) (1 + RTOL) (the derivation
    of that file's docstring); iteration counts need not match.  The chain and the sorted variant have the same q_index and
    the retime kernels never read opt_index: every output bit for bit."""
    import retime_convex_ref as cr
    from test_gpu_retime import RTOL
    from test_gpu_retime_convex import ALL as OUTPUTS, GAP_TOL, _against_reference_and_greedy
    assert GAP_TOL == RETIME_CONVEX_GAP
    views = rigs(name)
    got = {}
    for v in [views["original"]] + renumbered(views):
        paths, vm, am = rn.retime_inputs(v)
        assert np.isinf(vm).any() and np.isfinite(vm).any()
        with np.errstate(divide="ignore", invalid="ignore"):
            r = cr.retime_paths_convex_ref(paths, None, vm, am, 2, 16, GAP_TOL)
        got[v.variant] = g = _against_reference_and_greedy(v.h, paths, None, vm, am, 2, r, M=16)
        assert (g["status"] == 0).all() and (g["duration"] > 0).all()
    g0 = got["original"]
    for variant in rn.VARIANTS:
        g = got[variant]
        assert same(g["status"], g0["status"]), variant
        d, d0 = g["duration"], g0["duration"]
        gap = np.abs(d - d0) / np.minimum(d, d0)
        print(f"{name} {variant}: convex retime iterations {g['iters'].tolist()} / {g0['iters'].tolist()}, max |d - d_0| / min {gap.max():.3e}")
        WORST["retime_paths_convex duration across numberings (relative)"] = max(WORST.get("retime_paths_convex duration across numberings (relative)", 0.0), float(gap.max()))
        assert (np.abs(d - d0) <= GAP_TOL * np.minimum(d, d0) * (1 + RTOL)).all(), variant
    for k in OUTPUTS:
        assert same(got["chain"][k], got["sorted"][k]), k


def _payload_dict(pl):
    return dict(mass=pl[0], com=pl[1], inertia=pl[2])


@pytest.mark.parametrize("name", ALL)
def test_forward_dynamics(rigs, name):
    """A9: gto_forward_dynamics on the 20 states of A7 with seeded joint forces and the `full` payload, under four `locked`
    settings (rn.locked_lists: NULL, the explicit list equal to it, all but one, a seeded half whose free joints are
    contiguous in neither numbering).  fd_sets (csrc/gto_api.hip) takes NULL from opt_of_dof and fd_solve eliminates the free
    joints in ascending joint NUMBER.  Per view, against tests/forward_ref.py and the Jacobian-sum mass matrix on the original
    robot, permuted, at the bars of tests/test_gpu_forward.py: qdd 1e-11 cond(M_ff) max(1, |qdd|), round trip 1e-11, M 1e-11
    relative.  M_out's columns are independent rt_rnea passes and its symmetrisation is pairwise: the same bits in all
    three views after permuting back.  qdd: the chain and sorted variants have the same joint numbers and no slot is read,
    the same bits; original against renumbered only to the bar (another elimination order)."""
    import dynamics_ref as dr
    import forward_ref as fr
    views = rigs(name)
    v0 = views["original"]
    d0, ee = v0.desc, v0.desc.frame_index(v0.ee)
    q0, qd0, tau0, pl, locks0 = rn.forward_inputs(v0)
    n = len(q0)
    row = lambda i: (pl[0][i], pl[1][i], pl[2][i])  # noqa: E731
    out = {}
    for setting in rn.FORWARD_SETTINGS:
        free = fr.free_joints(d0, locks0[setting])
        assert free.any()
        ref = [fr.forward_dynamics(d0, q0[i], qd0[i], tau0[i], ee, row(i), locks0[setting]) for i in range(n)]
        got = {}
        for v in [v0] + renumbered(views):
            q, qd, tau, _, locks = rn.forward_inputs(v)
            qdd, status, Mv = v.h.forward_dynamics(q, qd, tau, _payload_dict(pl), locks[setting], want_mass_matrix=True)
            a, Ma = v.old(qdd, 1), v.old(v.old(Mv, 1), 2)
            assert (status == 0).all() and np.isfinite(a).all() and not a[:, ~free].any(), (setting, v.variant)
            worst_q = worst_rt = worst_M = 0.0
            for i in range(n):
                want, Mref = ref[i]
                Mff = Mref[np.ix_(free, free)]
                tol = 1e-11 * np.linalg.cond(Mff) * max(1.0, np.abs(want).max())
                worst_q = max(worst_q, np.abs(a[i] - want).max() / tol)
                back = dr.inverse_dynamics(d0, q0[i], qd0[i], a[i], ee, row(i))
                scale = max(1.0, np.abs(tau0[i]).max(), (np.abs(Mref) @ np.abs(a[i])).max())
                worst_rt = max(worst_rt, np.abs(back - tau0[i])[free].max() / scale)
                worst_M = max(worst_M, np.abs(Ma[i] - Mref).max() / np.abs(Mref).max())
            print(f"{name} {v.variant} locked={setting}: qdd error / tolerance {worst_q:.2e}, round trip {worst_rt:.2e}, M {worst_M:.2e}")
            for key, x in (("forward_dynamics qdd (of its tolerance)", worst_q), ("forward_dynamics round trip", worst_rt), ("forward_dynamics M (relative)", worst_M)):
                WORST[key] = max(WORST.get(key, 0.0), x)
            assert worst_q <= 1.0 and worst_rt <= 1e-11 and worst_M <= 1e-11, (setting, v.variant)
            got[v.variant] = (qdd, Mv, a, Ma)
        for variant in rn.VARIANTS:
            assert same(got[variant][3], got["original"][3]), (setting, variant)            # M_out: the same bits in every numbering
            assert setting != "null" or not same(got[variant][0], got["original"][0]), variant  # (the joint axes did move)
        assert same(got["chain"][0], got["sorted"][0]) and same(got["chain"][1], got["sorted"][1]), setting
        out[setting] = got
    for variant in ("original",) + rn.VARIANTS:   # the explicit list equal to the default is the default
        assert locks0["null"] is None and same(out["null"][variant][0], out["default"][variant][0]), variant
        assert not same(out["null"][variant][0], out["half"][variant][0])


ROLLOUT_STEPS = {"r3": 6, "r55": 6}


@pytest.mark.parametrize("mode", rn.ROLLOUT_MODES)
@pytest.mark.parametrize("name", ALL)
def test_track_rollout(rigs, name, mode):
    """A10: gto_track_rollout on three paths built on the original robot (rn.rollout_inputs), feedforward full, and the
    variant where one joint cannot hold; kp, kd and tau_max differ from joint to joint; locked = NULL and an explicit list
    that frees a parameter joint.  Per view against tests/forward_ref.rollout_batch on the ORIGINAL robot, permuted: steps,
    sat_steps and status equal, t bit for bit, q, qd, err_max, err_end within 16 d.  d = rn.ROLLOUT_D = 5.71e-10 is the largest
    difference of the restatement over these very cases between its two mass-matrix orderings (columns=False / True) and
    between the original and the renumbered description, measured on the CPU (tests/test_renumbered_robots_cpu.py holds the
    restatement to them); per case, orderings / numberings:
        r1 5.71e-10 / 4.96e-12   r9 1.47e-11 / 5.89e-13   r3 2.21e-14 / 8.89e-16   panda 2.17e-14 / 2.51e-16   r55 2.63e-11 / 1.65e-12
    (r1's with the list that frees a parameter joint: 1.68e-14 under the default).  No clip decision of the restatement comes
    within 1e-9 relative of its limit (the smallest margin: 2.4e-3).  The chain and the sorted variant: the same joint numbers,
    no slot is read, every output bit for bit."""
    views = rigs(name)
    v0 = views["original"]
    a0 = rn.rollout_inputs(v0, mode)
    tol = 16 * rn.ROLLOUT_D
    for lock in rn.ROLLOUT_LOCKS:
        want = rn.rollout_restatement(v0, a0, lock)
        assert want["clip_margin"].min() > 1e-9 and (want["status"] == 0).all()
        assert want["steps"].max() <= ROLLOUT_STEPS.get(name, 20) and want["steps"].min() >= 2
        if mode == "saturating":
            assert want["sat_steps"][0] > want["steps"][0] // 2
        got = {}
        for v in [v0] + renumbered(views):
            a = rn.rollout_inputs(v, mode)
            g = v.h.track_rollout(a["duration"], a["q"], a["qd"], a["qdd"], a["kp"], a["kd"], tau_max=a["tau_max"], dt=a["dt"],
                                  settle=a["settle"], n_samples=a["n_samples"], feedforward=a["feedforward"],
                                  model_payload={"mass": a["model"][0]}, plant_payload=_payload_dict(a["plant"]), locked=a["locks"][lock])
            got[v.variant] = g
            for k in ("steps", "sat_steps", "status"):
                assert np.array_equal(g[k], want[k]), (lock, v.variant, k, g[k], want[k])
            assert same(g["t"], want["t"]), (lock, v.variant)
            err = {k: float(np.abs((v.old(g[k], 2) if k in ("q", "qd") else g[k]) - want[k]).max()) for k in ("q", "qd", "err_max", "err_end")}
            print(f"{name} {mode} {lock} {v.variant}: steps {g['steps'].tolist()} sat {g['sat_steps'].tolist()} differences {err}, allowed {tol:.2e}")
            WORST["track_rollout q, qd, err_max, err_end"] = max(WORST.get("track_rollout q, qd, err_max, err_end", 0.0), max(err.values()))
            assert max(err.values()) <= tol, (lock, v.variant)
        for k in got["chain"]:
            assert same(got["chain"][k], got["sorted"][k]), (lock, k)
        assert not same(got["chain"]["q"], got["original"]["q"])


@pytest.mark.parametrize("name", ALL)
def test_retime_torque(rigs, name):
    """A11: gto_retime_paths_torque on the inputs of A8 with the `full` payload and tau_max drawn per joint on the original
    robot (rn.torque_limits: 1.5 to 3 times the largest static torque along the paths, +inf for a joint that carries none).
    Per view: tests/test_gpu_retime_torque._against_reference with the restatement on the ORIGINAL robot (it compares
    statuses and durations, recomputes the limits and the torques from the view's own outputs, and holds tau_out to
    gto_inverse_dynamics of the returned samples in that view, bit for bit).  Across views: equal statuses and durations
    within gap_tol, the rule of A8; the chain and the sorted variant bit for bit.  Where rn.TORQUE_ACTIVE says so at least one
    path has an active torque row, longer than the convex call's by more than 10 gap_tol; r3 and r55 have none at any seed
    (tests/test_renumbered_robots_cpu.py shows why), and there no path may be longer."""
    import retime_torque_ref as tr
    from test_gpu_retime import RTOL
    from test_gpu_retime_torque import ALL as OUTPUTS, GAP_TOL, _against_reference
    assert GAP_TOL == RETIME_CONVEX_GAP
    views = rigs(name)
    v0 = views["original"]
    fee, pl = v0.desc.frame_index(v0.ee), rn.torque_payload()
    paths0, vm0, am0 = rn.retime_inputs(v0)
    tm0 = rn.torque_limits(v0)
    assert np.isfinite(tm0).sum() >= 2 and len(set(tm0[np.isfinite(tm0)].tolist())) == np.isfinite(tm0).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = tr.retime_paths_torque_ref(v0.desc, fee, paths0, None, vm0, am0, tm0, pl, 2, 16, GAP_TOL)
    got = {}
    for v in [v0] + renumbered(views):
        paths, vm, am = rn.retime_inputs(v)
        tm = rn.torque_limits(v)
        assert same(v.old(tm, 0), tm0)
        g, convex = _against_reference(v.desc, fee, v.h, paths, None, vm, am, tm, pl, 2, r, M=16)
        got[v.variant] = g
        ok = g["status"] == 0
        active = ok & (g["duration"] > convex["duration"] * (1 + 10 * GAP_TOL))
        print(f"{name} {v.variant}: torque retime status {g['status'].tolist()} active {active.tolist()} iterations {g['iters'].tolist()}")
        assert active.any() == rn.TORQUE_ACTIVE[name], v.variant
    g0 = got["original"]
    ok = g0["status"] == 0
    for variant in rn.VARIANTS:
        g = got[variant]
        assert same(g["status"], g0["status"]), variant
        d, d0 = g["duration"][ok], g0["duration"][ok]
        gap = np.abs(d - d0) / np.minimum(d, d0)
        key = "retime_paths_torque duration across numberings (relative)"
        WORST[key] = max(WORST.get(key, 0.0), float(gap.max()))
        assert (np.abs(d - d0) <= GAP_TOL * np.minimum(d, d0) * (1 + RTOL)).all(), variant
    for k in OUTPUTS:
        assert same(got["chain"][k], got["sorted"][k]), k


# =================================================================================================== B. solves and sums over slots
def _close_blocks(a, b, rtol=1e-8):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-10 * max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("name", ALL)
def test_objective_and_obstacle_blocks(rigs, name):
    """B1: gto_eval_objective and gto_eval_obstacle_normal_eq; the blocks come in slot order."""
    views = rigs(name)
    v0 = views["original"]
    obj0 = [v0.h.eval_objective(0, v0.goals_all, v0.n_goals_ragged, S, v0.base, v0.Q0) for S in (v0.S, None)]
    A0, g0, ss0 = v0.h.eval_obstacle_normal_eq(0, v0.base, v0.Q0)
    assert ss0.max() > 0 and np.abs(A0[:, 2:]).max() > 0
    for v in renumbered(views):
        for S, want0 in zip((v.S, None), obj0):
            a = v.h.eval_objective(0, v.goals_all, v.n_goals_ragged, S, v.base, v.Q0)
            b = v.o.eval_objective(0, v.goals_all, v.n_goals_ragged, S, v.base, v.Q0)
            for k, (x, y) in enumerate(zip(a[:3], b[:3])):
                worst(f"eval_objective term {k} (relative)", x, y, True)
                np.testing.assert_allclose(x, y, rtol=1e-9, atol=1e-13)   # tests/test_gpu_parity.py:569
            np.testing.assert_array_equal(a[3], b[3])
            np.testing.assert_array_equal(a[3], want0[3])
            if v.variant == "chain":
                for x, y in zip(a, want0):
                    assert same(x, y)
            else:
                for x, y in zip(a[:3], want0[:3]):
                    np.testing.assert_allclose(x, y, rtol=1e-9, atol=1e-13)
        A, g, ss = v.h.eval_obstacle_normal_eq(0, v.base, v.Q0)
        Ao, go, sso = v.o.eval_obstacle_normal_eq(0, v.base, v.Q0)
        worst("eval_obstacle_normal_eq JtJ (relative to the largest entry)", A[:, 2:] / np.abs(Ao).max(), Ao[:, 2:] / np.abs(Ao).max())
        _close_blocks(A[:, 2:], Ao[:, 2:])                                 # tests/test_gpu_parity.py:572-574
        _close_blocks(g[:, 2:], go[:, 2:])
        np.testing.assert_allclose(ss, sso, rtol=1e-11, atol=1e-15)
        if v.variant == "chain":
            assert same(A, A0) and same(g, g0) and same(ss, ss0)
        else:   # the original's blocks permuted by sigma, at the relative tolerance of the oracle comparison
            assert (v.sigma != np.arange(len(v.sigma))).any()
            _close_blocks(v.slots_old(A, 2, 3)[:, 2:], A0[:, 2:])
            _close_blocks(v.slots_old(g, 2)[:, 2:], g0[:, 2:])
            np.testing.assert_allclose(ss, ss0, rtol=1e-11, atol=1e-15)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_trajectory_solve(rigs, name, ragged):
    """B2: gto_solve_batch and gto_solve_batch_device."""
    import torch
    views = rigs(name)
    v0 = views["original"]
    ref0 = v0.h.solve_batch(*v0.solve_args(ragged))
    for v in renumbered(views):
        args = v.solve_args(ragged)
        got = v.h.solve_batch(*args)
        Qg, dQg, fg, itg, stg = got
        Qo, dQo, fo, ito, sto = v.o.solve_batch(*args, n_threads=v.nt)
        print(f"{name} {v.variant} ragged={ragged}: iterations gpu {itg.tolist()} oracle {ito.tolist()} max |Q - Q_oracle| {np.abs(Qg - Qo).max():.3e}")
        worst("solve_batch Q", Qg, Qo)
        worst("solve_batch cost (relative)", fg, fo, True)
        np.testing.assert_array_equal(itg, ito)                            # tests/test_gpu_parity.py:577-582
        np.testing.assert_array_equal(stg, sto)
        assert np.isin(stg, OK).all() and (itg > 1).all()
        np.testing.assert_allclose(Qg, Qo, rtol=0, atol=1e-6)
        np.testing.assert_allclose(fg, fo, rtol=1e-8)
        if v.variant == "chain":
            for x, y, ax in zip(got, ref0, (1, 1, None, None, None)):
                assert same(x if ax is None else v.old(x, ax), y)
        # the device entry point, bit for bit (tests/test_gpu_parity.py::test_device_entry_point_on_caller_stream)
        B, nd, T = v.B, v.desc.ndof, v.T
        n_max = args[2].shape[1]
        inp = [cu(np.zeros(B, np.int32)), cu(v.qc), cu(args[2]), cu(args[3]), cu(np.tile(v.S.reshape(1, 16), (B, 1))), cu(v.base), cu(v.Q0)]
        out = [torch.empty((B, nd, T), dtype=torch.float64, device="cuda:0"), torch.empty((B, nd, T - 1), dtype=torch.float64, device="cuda:0"),
               torch.empty(B, dtype=torch.float64, device="cuda:0"), torch.empty(B, dtype=torch.int32, device="cuda:0"),
               torch.empty(B, dtype=torch.int32, device="cuda:0")]
        stream = torch.cuda.Stream("cuda:0")
        torch.cuda.synchronize()
        v.h.solve_batch_device(B, n_max, *[x.data_ptr() for x in inp + out], stream.cuda_stream)
        stream.synchronize()
        for x, y in zip(got, out):
            assert same(x, y.cpu().numpy())


@pytest.mark.parametrize("name", NARROW)
def test_ik_to_point_goals(rigs, name):
    """B3: gto_solve_ik_batch with and without a scene; instance 0 starts with one optimised joint below and one above its
    limits, so the clip of the seed has to use each joint's own bounds."""
    views = rigs(name)
    v0 = views["original"]
    for sid in (None, 0):
        ref0 = v0.h.solve_ik_batch(sid, rn.ik_start(v0), v0.goals[:, 0], v0.base, max_iter=rn.IK_MAX_ITER)
        for v in renumbered(views):
            q0 = rn.ik_start(v)
            qi, fi, iti, sti = got = v.h.solve_ik_batch(sid, q0, v.goals[:, 0], v.base, max_iter=rn.IK_MAX_ITER)
            qo, fo, ito, sto = v.o.solve_ik_batch(sid, q0, v.goals[:, 0], v.base, max_iter=rn.IK_MAX_ITER, n_threads=v.nt)
            worst("solve_ik_batch q", qi, qo)
            np.testing.assert_array_equal(iti, ito)                        # tests/test_gpu_parity.py:585-589
            np.testing.assert_array_equal(sti, sto)
            assert np.isin(sti, OK).all()
            np.testing.assert_allclose(qi, qo, rtol=0, atol=1e-6)
            np.testing.assert_allclose(fi, fo, rtol=1e-8, atol=1e-12)      # tests/test_gpu_small_robots.py:161
            opt = v.desc.opt_index
            assert (qi[:, opt] >= v.desc.lower[opt]).all() and (qi[:, opt] <= v.desc.upper[opt]).all()
            par = v.desc.param_index
            assert same(qi[:, par], q0[:, par])
            # no iteration: the clipped seed, every optimised joint by its own bounds
            q1, _, it1, st1 = v.h.solve_ik_batch(sid, q0, v.goals[:, 0], v.base, max_iter=0)
            clipped = q0.copy()
            clipped[:, opt] = np.clip(q0[:, opt], v.desc.lower[opt], v.desc.upper[opt])
            assert (it1 == 0).all() and same(q1, clipped) and not same(clipped[0], q0[0])
            if v.variant == "chain":
                for x, y, ax in zip(got, ref0, (1, None, None, None)):
                    assert same(x if ax is None else v.old(x, ax), y), (sid, "chain")


@pytest.mark.parametrize("goal_kind", [pref.GTO_IK_GOAL_QUATERNION, pref.GTO_IK_GOAL_RPY])
@pytest.mark.parametrize("name", NARROW)
def test_ik_to_pose_goals(rigs, name, goal_kind):
    """B3: gto_solve_ik_pose_batch against tests/ik_pose_ref.py as tests/test_gpu_ik_pose_cases.py holds it (iterations and
    status equal, q to 1e-9, cost to rtol 1e-10; quoted from tests/test_gpu_small_robots.py:176-179)."""
    views = rigs(name)
    v0 = views["original"]
    goals = sr.pose_goals(v0, goal_kind)
    ref0 = v0.h.solve_ik_pose_batch(goal_kind, None, v0.qc, goals, None, max_iter=rn.POSE_MAX_ITER)
    for v in renumbered(views):
        got = v.h.solve_ik_pose_batch(goal_kind, None, v.qc, goals, None, max_iter=rn.POSE_MAX_ITER)
        qr, fr, itr, str_ = sr.pose_restatement(v, v.o, goal_kind, max_iter=rn.POSE_MAX_ITER)
        worst("solve_ik_pose_batch q", got[0], qr)
        np.testing.assert_array_equal(got[2], itr)
        np.testing.assert_array_equal(got[3], str_)
        np.testing.assert_allclose(got[0], qr, rtol=0, atol=1e-9)
        np.testing.assert_allclose(got[1], fr, rtol=1e-10, atol=1e-15)
        if v.variant == "chain":
            for x, y, ax in zip(got, ref0, (1, None, None, None)):
                assert same(x if ax is None else v.old(x, ax), y)
        # with the scene: a regular end, and the cost is the pose term plus the oracle's collision term at the returned q
        qs, fs, its, sts = v.h.solve_ik_pose_batch(goal_kind, 0, v.qc, goals, v.base, max_iter=rn.POSE_MAX_ITER)
        assert np.isfinite(qs).all() and np.isin(sts, OK).all()
        Tq = v.o.eval_fk(qs)[:, v.desc.frame_index(v.ee)]
        val = np.stack([v.o.eval_points(0, qs[b:b + 1], v.base[b], use_obs=True)[2].sum() for b in range(v.B)])
        want = np.array([pref.pose_term(goal_kind, Tq[b], goals[b]) for b in range(v.B)]) + v.opts.w_obstacle * val
        np.testing.assert_allclose(fs, want, rtol=1e-9, atol=1e-13)       # tests/test_gpu_small_robots.py:186


@pytest.mark.parametrize("name", NARROW)
def test_base_placement(rigs, name):
    """B4: gto_solve_base_batch with gto_eval_base_objective (tolerances: tests/test_gpu_small_robots.py:252-258)."""
    views = rigs(name)
    v0 = views["original"]
    ng, n_max = v0.n_goals_ragged, rn.N_MAX
    ref0 = v0.h.solve_base_batch(v0.qc, v0.goals_all, ng, 0.01, max_iter=rn.BASE_MAX_ITER)
    live = ng[:, None] > np.arange(n_max)
    for v in renumbered(views):
        got = yg, qg, fg, itg, stg = v.h.solve_base_batch(v.qc, v.goals_all, ng, 0.01, max_iter=rn.BASE_MAX_ITER)
        yo, qo, fo, ito, sto = v.o.solve_base_batch(v.qc, v.goals_all, ng, 0.01, max_iter=rn.BASE_MAX_ITER, n_threads=v.nt)
        worst("solve_base_batch y", yg, yo)
        worst("solve_base_batch q", qg[live], qo[live])
        np.testing.assert_array_equal(itg, ito)
        np.testing.assert_array_equal(stg, sto)
        assert np.isin(stg, OK).all()
        np.testing.assert_allclose(fg, fo, rtol=1e-7, atol=1e-12)
        np.testing.assert_allclose(yg, yo, rtol=0, atol=1e-6)
        np.testing.assert_allclose(qg[live], qo[live], rtol=0, atol=1e-6)
        assert same(qg[~live], np.broadcast_to(v.qc[:, None], qg.shape)[~live])        # rows past a set's goals: qc
        par = v.desc.param_index
        assert same(qg[:, :, par], np.broadcast_to(v.qc[:, None], qg.shape)[:, :, par])  # parameter joints as given
        fe_g = v.h.eval_base_objective(yg, qg, v.goals_all, ng, 0.01)
        fe_o = v.o.eval_base_objective(yg, qg, v.goals_all, ng, 0.01)
        worst("eval_base_objective (relative)", fe_g, fe_o, True)
        np.testing.assert_allclose(fe_g, fe_o, rtol=1e-7, atol=1e-12)
        np.testing.assert_allclose(fe_g, fg, rtol=1e-7, atol=1e-12)
        if v.variant == "chain":
            for x, y, ax in zip(got, ref0, (None, 2, None, None, None)):
                assert same(x if ax is None else v.old(x, ax), y)
            assert same(fe_g, v0.h.eval_base_objective(ref0[0], ref0[1], v0.goals_all, ng, 0.01))


@pytest.mark.parametrize("name", NARROW)
def test_base_report(rigs, name):
    """B4: gto_base_report_device against tests/base_chain_ref.py (ERR_POS_TOL, ERR_ROT_TOL of tests/test_gpu_base_chain.py).
    Nothing is summed over joints here: the same bits in both variants."""
    import copy
    from test_gpu_base_chain import ERR_POS_TOL, ERR_ROT_TOL, occupancy, run_report, same_grid
    views = rigs(name)
    v0 = views["original"]
    d0, B, n_max = v0.desc, 5, 3
    case = bref.report_case(v0.o, d0, B, n_max, 300 + ALL.index(name))
    occ = occupancy(case.cloud, epsilon=case.epsilon)
    same_grid(occ, case.grid)
    w_ep, w_er = bref.report(v0.o, d0.frame_index(v0.ee), d0.frame_index(v0.gripper), case.goals, case.n_goals, case.y, case.q, fill=-7.0)
    w_col = bref.collisions(case.grid, case.foot, case.y, case.qc)
    live = case.n_goals[:, None] > np.arange(n_max)
    g0 = run_report(v0.h, occ, case, B, n_max)
    for v in renumbered(views):
        pc = copy.copy(case)
        pc.qc, pc.q = v.new(case.qc, 1), v.new(case.q, 2)
        g = ep, er, col, ff = run_report(v.h, occ, pc, B, n_max)
        for x, y in zip(g, g0):
            assert same(x, y), v.variant
        worst("base_report err_pos", ep[live], w_ep[live])
        worst("base_report err_rot (degrees)", er[live], w_er[live])
        assert (ep[~live] == -7.0).all() and (er[~live] == -7.0).all()
        np.testing.assert_allclose(ep[live], w_ep[live], rtol=0, atol=ERR_POS_TOL)
        np.testing.assert_allclose(er[live], w_er[live], rtol=0, atol=ERR_ROT_TOL)
        np.testing.assert_array_equal(col, w_col)
        assert ff[0] == bref.first_free(w_col)
    occ.close()


def _seed_case(v0):
    """renumbered_robots.seed_goalset_case on the original robot; the parameter joints of the solutions are away from qc's."""
    qc, qs, goals, n_goals, accept, sid, base = rn.seed_goalset_case(v0.case)
    par = v0.desc.param_index
    assert np.abs(qs[:, :, par] - qc[:, None, par]).min() > 0
    return qc, qs, goals, n_goals, accept, sid, base


def _seed_case_in(v, case):
    qc, qs, goals, n_goals, accept, sid, base = case
    return v.new(qc, 1), v.new(qs, 2), goals, n_goals, accept, sid, base


@pytest.mark.parametrize("name", NARROW)
def test_seed_choice(rigs, name):
    """B5: gto_seed_goalsets_device as tests/test_gpu_seed_waves.check_seeds holds it against the oracle-scored restatement on
    the renumbered robot (costs to 1e-12, distances to 1e-14, the choice exact on the kernel's own scores, the seed built
    from it bit for bit: parameter rows pinned from qc, optimised rows interpolated), and against the original robot's call."""
    import torch
    from test_gpu_grasp_chain import run_seeds, same_bits
    from test_gpu_seed_waves import check_seeds, clearly_first, oracle_seeds
    views = rigs(name)
    v0 = views["original"]
    case0 = _seed_case(v0)
    for f32 in (True, False):
        g0 = run_seeds(v0.h, torch, v0.T, *case0, True, f32)
        for v in renumbered(views):
            case = _seed_case_in(v, case0)
            want = oracle_seeds(v, case, f32)
            left_out, w = check_seeds(v, case, want, True, f32)
            WORST["seed_goalsets seed_cost (relative)"] = max(WORST.get("seed_goalsets seed_cost (relative)", 0.0), w)
            assert left_out <= 1 + sr.seed_cost_ties(want)
            g = run_seeds(v.h, torch, v.T, *case, True, f32)
            for k in ("goals_out", "n_goals_out", "n_accepted", "seed_cost"):
                assert same(g[k], g0[k]), (v.variant, k)
            # seed_dist is |q_0 - q_{T-1}| of the candidate, a sum of squares over the actuated joints in joint order
            # (gto_seed.h, seed_select_body's loop over dq): renumbering reorders the sum in both variants, so it is held to
            # the original's at the 1e-14 check_seeds holds it to the oracle at (RT_DIST); the choice and the seed built
            # from it are compared wherever no scorer within the tolerances could choose otherwise
            # (test_gpu_seed_waves.clearly_first)
            np.testing.assert_allclose(g["seed_dist"], g0["seed_dist"], rtol=1e-14, atol=0)
            for b in range(v.B):
                na = int(g0["n_accepted"][b])
                if na == 0 or clearly_first(g0["seed_cost"][b, :na], g0["seed_dist"][b, :na]):
                    assert g["seed_index"][b] == g0["seed_index"][b], (v.variant, b)
                    assert same_bits(v.old(g["Q0"][b], 0), g0["Q0"][b]), (v.variant, b)


@pytest.mark.parametrize("name", NARROW)
def test_three_seeds(rigs, name):
    """B5: gto_seed_goalsets_multi_device with three seeds against tests/multistart_ref.seed_slots scored by the handle's own
    gto_plan_cost, as tests/test_gpu_multistart.py holds it."""
    import torch
    from test_gpu_grasp_chain import run_seeds
    from test_gpu_multistart import check_slots, run_seeds_multi
    views = rigs(name)
    case0 = _seed_case(views["original"])
    K = 3
    for v in renumbered(views):
        qc, qs, goals, n_goals, accept, sid, base = case = _seed_case_in(v, case0)
        plain = run_seeds(v.h, torch, v.T, *case, True, True)
        got = run_seeds_multi(v.h, v.T, K, *case, True, True)
        for b in range(v.B):
            r = mref.seed_slots(qc[b], goals[b], n_goals[b], qs[b], accept[b], v.T, v.offset, v.desc.param_index, True, True,
                                lambda plans, b=b: v.h.plan_cost(int(sid[b]), plans, base[b])[0], K)
            check_slots(got, plain, b, r, K, v.T)


@pytest.mark.parametrize("name", NARROW)
def test_plan_report(rigs, name):
    """B6: gto_plan_report_device against gto_eval_objective and gto_ik_report_device, as
    tests/test_gpu_multistart.py::test_plan_report_against_eval_objective_and_ik_report does."""
    import torch
    from test_gpu_grasp_chain import dev_empty
    from test_gpu_multistart import run_report
    views = rigs(name)
    v0 = views["original"]
    g0 = run_report(v0.h, v0.goals_all, v0.n_goals_ragged, v0.S, v0.Q0)
    for v in renumbered(views):
        B, T = v.B, v.T
        f_goal, _, _, argmin = v.h.eval_objective(0, v.goals_all, v.n_goals_ragged, v.S, v.base, v.Q0)
        got = run_report(v.h, v.goals_all, v.n_goals_ragged, v.S, v.Q0)
        assert got["goal_index"].tolist() == argmin.tolist()
        np.testing.assert_allclose(got["goal_cost"], f_goal, rtol=1e-12, atol=0)     # tests/test_gpu_multistart.py:193
        outs = [dev_empty((B,), torch.float64) for _ in range(2)]
        keep = [cu(v.Q0[:, :, T - 1]), cu(v.goals_all[np.arange(B), argmin])]
        torch.cuda.synchronize()
        v.h.ik_report_device(B, None, keep[0].data_ptr(), keep[1].data_ptr(), None, 0.01, 5.0, 5.0, outs[0].data_ptr(), outs[1].data_ptr())
        torch.cuda.synchronize()
        assert same(got["err_pos"], outs[0].cpu().numpy()) and same(got["err_rot"], outs[1].cpu().numpy())
        for k in ("goal_index", "err_pos", "err_rot"):   # nothing summed over slots
            assert same(got[k], g0[k]), (v.variant, k)
        if v.variant == "chain":
            assert same(got["goal_cost"], g0["goal_cost"])
        else:
            np.testing.assert_allclose(got["goal_cost"], g0["goal_cost"], rtol=1e-12, atol=0)


def _lift_device(v, plans, sid, base):
    import torch
    B, K = plans.shape[0], rn.LIFT_K
    f64, i32 = torch.float64, torch.int32
    new = lambda shape, dt: torch.full(shape, -7, dtype=dt, device="cuda:0")
    out = dict(path=new((B, v.desc.ndof, K + 1), f64), goals=new((B, K, 4, 4), f64), err_pos=new((B, K), f64), err_rot=new((B, K), f64),
               iters=new((B, K), i32), status=new((B, K), i32), reached=new((B,), i32))
    keep = [cu(plans), cu(np.full(B, sid, np.int32)), cu(base)]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    v.h.retrieve_lift_device(B, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), rn.LIFT_DIRECTION, rn.LIFT_DISTANCE, K,
                             v.closed_joints, v.closed_values, rn.LIFT_MAX_ITER, rr.POS_TOL, rr.ROT_TOL_DEG, out["path"].data_ptr(),
                             out["goals"].data_ptr(), out["err_pos"].data_ptr(), out["err_rot"].data_ptr(), out["iters"].data_ptr(),
                             out["status"].data_ptr(), out["reached"].data_ptr(), st.cuda_stream)
    st.synchronize()
    return {k: x.cpu().numpy() for k, x in out.items()}


LIFT_FIELDS = ("path", "goals", "err_pos", "err_rot", "iters", "status", "reached")


@pytest.mark.parametrize("name", NARROW)
def test_retrieve_lift(rigs, name):
    """B7: gto_retrieve_lift and gto_retrieve_lift_device along a slanted line, with per-plan non-zero bases, a scene, closed
    parameter joints at distinct non-zero values and one plan that ends with an optimised joint out of its limits: bit for
    bit the host-driven chain (retrieve_ref.lift_chain over the handle) in both variants, and the oracle chain with equal
    counts to 1e-6 rad (tests/test_gpu_retrieve.py:126-130).  reached below K is an answer like any other, and it is compared."""
    views = rigs(name)
    v0 = views["original"]
    results = {}
    for v in [v0] + renumbered(views):
        plans, scene = rn.lift_plans(v, v0.o.eval_fk)
        sid = 0
        if scene is not None:
            v.h.set_scene(1, *scene)
            v.o.set_scene(1, *scene)
            sid = 1
        base = rn.lift_bases(v, len(plans))
        args = (rn.LIFT_DISTANCE, rn.LIFT_K, rn.LIFT_DIRECTION, v.closed_joints, v.closed_values)
        kw = dict(scene_id=sid, base_pos=base, max_iter=rn.LIFT_MAX_ITER)
        got = v.h.retrieve_lift(plans, *args, **kw)
        host = rr.lift_chain(v.h, v.desc, v.ee, plans, *args, **kw)
        assert same(got["goals"], host["goals"]), "RT0 or the goal expression"
        for k in ("path", "iters", "status", "reached"):
            assert same(got[k], host[k]), (v.variant, k)
        dev = _lift_device(v, plans, sid, base)
        for k in LIFT_FIELDS:
            assert same(dev[k], got[k]), (v.variant, k)
        want = rr.lift_chain(v.o, v.desc, v.ee, plans, *args, **kw)
        print(f"{name} {v.variant}: lift iterations {got['iters'].ravel().tolist()} reached {got['reached'].tolist()} "
              f"max |path - oracle| {np.abs(got['path'] - want['path']).max():.3e}")
        worst("retrieve_lift path", got["path"], want["path"])
        assert np.array_equal(got["iters"], want["iters"]) and np.array_equal(got["status"], want["status"])
        np.testing.assert_allclose(got["path"], want["path"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(got["goals"], want["goals"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(got["err_pos"], want["err_pos"], rtol=0, atol=1e-9)
        assert np.array_equal(got["reached"], want["reached"])
        # the closed joints hold their own values in every column, every other parameter joint the plan's last value
        cj = v.closed_joints
        assert (got["path"][:, cj, :] == np.asarray(v.closed_values)[None, :, None]).all()
        rest = [int(j) for j in v.desc.param_index if int(j) not in cj]
        assert same(got["path"][:, rest, :], np.repeat(plans[:, rest, -1:], rn.LIFT_K + 1, axis=2))
        results[v.variant] = got
    j = int(v0.desc.opt_index[1])   # out of limits in the last plan: column 0 keeps it, the columns after it are inside
    p0 = results["original"]["path"]
    assert p0[-1, j, 0] > v0.desc.upper[j] and (p0[-1, j, 1:] <= v0.desc.upper[j]).all()
    for k in LIFT_FIELDS:
        x = results["chain"][k]
        assert same(views["chain"].old(x, 1) if k == "path" else x, results["original"][k]), k
    for k in ("iters", "status", "reached"):
        assert same(results["sorted"][k], results["original"][k]), k
