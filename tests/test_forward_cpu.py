"""tests/forward_ref.py, the yardstick of gto_forward_dynamics and gto_track_rollout, held against physics rather than against
itself, and the host-only rules of the Python layers (no GPU here).

  1. Round trip: ID(q, qd, FD(q, qd, tau)) == tau on the free joints, for the 11 robots of tests/dynamics_cases.py on the
     seeded states and payloads of tests/test_dynamics_cpu.py, to 1e-11 relative to max(1, |tau|_inf, (|M| |qdd|)_inf), the
     project's inverse-dynamics tolerance.  FD takes M from the Jacobian sum, ID is the recursion: two formulations.
  2. Order of the integrator: free motion under gravity (no gains, no feedforward, no torque limit, fingers locked)
     conserves T + V, and the drift over a fixed time falls by 2^4 when the step is halved.
  3. A robot fed its holding torque stays.
  4. The zero-order hold of the controller makes the tracking error first order in dt.
  5. The two payloads matter and the clip counts.
  6. Host-only argument rules, symbols and bindings.

Every rollout here is at most 100 steps (the numpy restatement costs about 25 ms per step on Panda).  Check 4 therefore runs
its three legs (dt = 4, 2, 1 ms) over the first 0.1 s of the 0.3 s move, not over all of it: 25, 50 and 100 steps.
"""
import inspect
import json
import os

import numpy as np
import pytest

import dynamics_cases as dc
import dynamics_ref as dr
import forward_ref as fr
from test_dynamics_cpu import FEWER_STATES, N_STATES, mass_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
ROUND_TRIP = 1e-11


@pytest.fixture(scope="module")
def panda():
    desc, ee, _, _ = dc.robot("panda")
    with open(os.path.join(ROOT, "grasptrajopt_amd", "data", "panda_cfg.json")) as fh:
        cfg = json.load(fh)
    return desc, desc.frame_index(ee), np.array(cfg["default_pose"], dtype=np.float64)


@pytest.mark.parametrize("name", dc.NAMES)
def test_round_trip(name):
    desc, ee, _, _ = dc.robot(name)
    ee = desc.frame_index(ee)
    q, qd, _ = dr.in_limit_states(desc, N_STATES, seed=5)
    pl = dc.payloads(N_STATES, seed=6)["full"]
    tau = np.random.default_rng(7).uniform(-20.0, 20.0, q.shape)
    worst = 0.0
    for i in range(FEWER_STATES.get(name, N_STATES)):
        payload = None if i % 2 == 0 else (pl[0][i], pl[1][i], pl[2][i])
        M = mass_matrix(desc, q[i], ee, payload)
        for locked in (None, np.zeros(desc.ndof)):
            free = fr.free_joints(desc, locked) & (np.diag(M) > 0)  # a joint that moves no mass cannot be free
            qdd, M2 = fr.forward_dynamics(desc, q[i], qd[i], tau[i], ee, payload, ~free)
            assert np.isfinite(qdd).all() and (qdd[~free] == 0).all() and np.array_equal(M, M2)
            back = dr.inverse_dynamics(desc, q[i], qd[i], qdd, ee, payload)
            scale = max(1.0, np.abs(tau[i]).max(), (np.abs(M) @ np.abs(qdd)).max())
            worst = max(worst, np.abs(back - tau[i])[free].max() / scale if free.any() else 0.0)
    print(f"{name}: round trip {worst:.3e}")
    assert worst <= ROUND_TRIP
    # a free joint that moves no mass: NaN, not a wild number
    massless = fr.named_joints(desc) & ~(np.diag(mass_matrix(desc, q[0], ee, None)) > 0)
    if massless.any():
        assert np.isnan(fr.forward_dynamics(desc, q[0], qd[0], tau[0], ee, None, np.zeros(desc.ndof))[0]).all()


def free_fall(desc, ee, q0, qd0, T, h):
    """The state after T seconds of free motion from (q0, qd0) at step h, and the step count."""
    ref = np.stack([q0, q0]), np.stack([qd0, qd0]), np.zeros((2, desc.ndof))
    out = fr.rollout(desc, ee, T, *ref, kp=0.0, kd=0.0, tau_max=np.inf, dt=h, n_samples=2, feedforward=0)
    assert out["status"] == fr.CONVERGED and out["sat_steps"] == 0 and out["t"][1] == out["steps"] * h
    return out["q"][1], out["qd"][1], out["steps"]


def test_integrator_is_fourth_order(panda):
    desc, ee, _ = panda
    q, qd, _ = dr.in_limit_states(desc, 1, seed=9)
    free = fr.free_joints(desc)
    q0, qd0 = q[0], np.where(free, 0.5 * qd[0], 0.0)
    E0 = fr.energy(desc, q0, qd0, ee)
    drift, steps = [], []
    for h in (0.02, 0.01, 0.005):
        q1, qd1, K = free_fall(desc, ee, q0, qd0, 0.2, h)
        drift.append(fr.energy(desc, q1, qd1, ee) - E0)
        steps.append(K)
    order = [np.log2(drift[i] / drift[i + 1]) for i in range(2)]
    print(f"energy drift {drift} over {steps} steps, observed order {order}, E0 {E0:.4f}")
    assert steps == [10, 20, 40]
    assert min(abs(d) for d in drift) >= 1e3 * EPS * abs(E0) * max(steps)  # far above the round-off of the energy itself
    assert all(abs(o - 4.0) <= 0.25 for o in order)


def test_a_robot_fed_its_holding_torque_stays(panda):
    desc, ee, pose = panda
    payload = (1.5, np.array([0.0, 0.02, 0.1]), None)
    K = 20
    ref = np.stack([pose, pose]), np.zeros((2, desc.ndof)), np.zeros((2, desc.ndof))
    out = fr.rollout(desc, ee, 0.04, *ref, kp=0.0, kd=0.0, tau_max=np.inf, dt=2e-3, n_samples=5, feedforward=1,
                     model_payload=payload, plant_payload=payload)
    g = dr.inverse_dynamics(desc, pose, 0 * pose, 0 * pose, ee, payload)
    print(f"holding: err_max {out['err_max']:.3e}, |g|_inf {np.abs(g).max():.2f}")
    assert out["status"] == fr.CONVERGED and out["steps"] == K
    assert out["err_max"] <= ROUND_TRIP * max(1.0, np.abs(g).max()) * K
    assert np.array_equal(out["t"], np.array([0, 5, 10, 15, 20]) * 2e-3)  # samples at steps floor(m K / (Mo - 1))


KP = np.array([600.0, 600, 600, 600, 250, 150, 50, 0, 0])
KD = np.array([50.0, 50, 50, 20, 20, 20, 10, 0, 0])


def quintic_reference(pose, delta, T, t_end, M):
    """Samples of pose + delta s(t / T), s the quintic 10 x^3 - 15 x^4 + 6 x^5, at linspace(0, t_end, M)."""
    x = np.linspace(0.0, t_end, M)[:, None] / T
    s = 10 * x ** 3 - 15 * x ** 4 + 6 * x ** 5
    sd = (30 * x ** 2 - 60 * x ** 3 + 30 * x ** 4) / T
    sdd = (60 * x - 180 * x ** 2 + 120 * x ** 3) / T ** 2
    return pose + s * delta, sd * delta, sdd * delta


def test_zero_order_hold_is_first_order(panda):
    desc, ee, pose = panda
    delta = np.where(fr.free_joints(desc), 0.05, 0.0)
    ref = quintic_reference(pose, delta, 0.3, 0.1, 101)  # the first 0.1 s of the move (see the head of the file)
    errs = []
    for dt in (4e-3, 2e-3, 1e-3):
        out = fr.rollout(desc, ee, 0.1, *ref, kp=KP, kd=KD, tau_max=desc.effort, dt=dt, n_samples=3, feedforward=2)
        assert out["status"] == fr.CONVERGED and out["sat_steps"] == 0 and out["steps"] <= 100
        errs.append(out["err_max"])
    print(f"zero-order hold: err_max {errs}, ratios {errs[0] / errs[1]:.3f} {errs[1] / errs[2]:.3f}")
    assert 1.8 <= errs[0] / errs[1] <= 2.2 and 1.8 <= errs[1] / errs[2] <= 2.2


def test_payloads_matter_and_the_clip_counts(panda):
    desc, ee, pose = panda
    two_kg = (2.0, np.array([0.0, 0.0, 0.1]), None)
    ref = np.stack([pose, pose]), np.zeros((2, desc.ndof)), np.zeros((2, desc.ndof))
    kw = dict(kp=KP, kd=KD, dt=2e-3, n_samples=4, feedforward=1, plant_payload=two_kg)
    known = fr.rollout(desc, ee, 0.1, *ref, tau_max=desc.effort, model_payload=two_kg, **kw)
    unknown = fr.rollout(desc, ee, 0.1, *ref, tau_max=desc.effort, model_payload=None, **kw)
    assert known["status"] == unknown["status"] == fr.CONVERGED and known["steps"] == 50
    assert known["sat_steps"] == 0 and unknown["sat_steps"] == 0
    print(f"2 kg modelled: err_end {known['err_end']:.3e}; unmodelled: {unknown['err_end']:.3e}")
    assert unknown["err_end"] > known["err_end"] and unknown["err_end"] > 1e-5
    g = dr.inverse_dynamics(desc, pose, 0 * pose, 0 * pose, ee, two_kg)
    j = int(np.argmax(np.abs(g[:7])))
    weak = np.asarray(desc.effort, dtype=np.float64).copy()
    weak[j] = 0.5 * abs(g[j])  # this joint cannot hold
    clipped = fr.rollout(desc, ee, 0.1, *ref, tau_max=weak, model_payload=two_kg, **kw)
    print(f"joint {j} holds {g[j]:.2f} N m, limited to {weak[j]:.2f}: sat_steps {clipped['sat_steps']}, err_end {clipped['err_end']:.3e}")
    assert clipped["status"] == fr.CONVERGED and clipped["sat_steps"] == clipped["steps"] == 50
    assert clipped["err_end"] > known["err_max"]


def test_reference_interpolation():
    """The Hermite interpolant reproduces a cubic and its derivative exactly (to round-off), holds the last sample past the
    end, and a zero duration is the last sample at once."""
    M, T = 6, 0.8
    t = np.linspace(0, T, M)
    c = np.array([[0.3, -1.0, 2.0, 0.7], [-0.2, 0.5, -1.5, 1.1]])  # two joints
    q = np.stack([np.polyval(c[j], t) for j in range(2)], axis=1)
    qd = np.stack([np.polyval(np.polyder(c[j]), t) for j in range(2)], axis=1)
    qdd = np.stack([np.polyval(np.polyder(c[j], 2), t) for j in range(2)], axis=1)
    for x in (0.0, 0.013, 0.16, 0.5, 0.79999, 0.8 - 1e-15):
        a, b, cc = fr.reference_at(x, T, q, qd, qdd)
        for j in range(2):
            assert abs(a[j] - np.polyval(c[j], x)) < 1e-14 and abs(b[j] - np.polyval(np.polyder(c[j]), x)) < 1e-13
            assert abs(cc[j] - np.polyval(np.polyder(c[j], 2), x)) < 1e-13  # linear in t for a cubic
    for x in (T, 1.0, 50.0):
        a, b, cc = fr.reference_at(x, T, q, qd, qdd)
        assert np.array_equal(a, q[-1]) and not b.any() and not cc.any()
    a, b, cc = fr.reference_at(0.0, 0.0, q, qd, qdd)
    assert np.array_equal(a, q[-1]) and not b.any()


def test_the_rollout_cases_cover_the_workgroup_layouts():
    """tests/test_gpu_forward.py's restatement of track_group_lanes / track_paths_per_block against the header's own functions
    would need the GPU library; here: the formula on the robots the GPU test names, and what the smallest ones are there for."""
    import test_gpu_forward as tg
    assert tg.track_layout(1, 1) == (16, 4) and tg.track_layout(32, 31) == (8, 1) and tg.track_layout(12, 9) == (16, 2)
    # one path at G lanes: (15 F G + ndof^2 + 15 ndof) 8 + 16 bytes of the 63488 a workgroup has
    assert (15 * 32 * 16 + 31 * 31 + 15 * 31) * 8 + 16 > 63488 >= (15 * 32 * 8 + 31 * 31 + 15 * 31) * 8 + 16
    tg.test_the_rollout_robots_cover_the_layouts()
    four = [n for n, lay in tg.ROLLOUT_LAYOUTS.items() if lay == (16, 4)]
    assert sorted(four) == ["chain_1", "ee_above_joints", "prismatic_only", "root_joint"]
    assert tg.B == 5 and -(-tg.B // 4) == 2 and tg.B % 4 == 1  # a full workgroup of four paths and one with a single valid group
    steps = np.ceil((tg.DURATIONS + 0.01) / tg.DT)
    assert len(set(steps.tolist())) == 5  # five different step counts share the barriers


@pytest.mark.parametrize("name", ["chain_1", "panda"])
def test_locked_joints_in_the_restatement(name):
    """The `locked` rules of include/gto_solver.h as tests/forward_ref.py states them, on the cases of
    tests/test_gpu_forward.test_rollout_with_locked_joints: a locked joint stands at its first reference position whatever its
    reference does later (a NaN there included), only a NaN in that first position fails the path, and with every joint locked
    nothing moves and nothing is in error."""
    import test_gpu_forward as tg
    c = tg.locked_case(name)
    res = {}
    for setting in ("all", "moving_nan", "first_nan"):
        lk, q, qd, qdd = tg.locked_inputs(c, setting)
        res[setting] = w = tg.locked_restatement(c, lk, q, qd, qdd)
        free = fr.free_joints(c["desc"], lk)
        good = w["status"] == 0
        assert good.tolist() == [True, setting != "first_nan", True, True, True] and w["steps"][good].max() <= tg.LOCKED_MAX_STEPS[name]
        assert np.array_equal(w["q"][good][:, :, ~free], np.broadcast_to(q[good][:, :1, ~free], w["q"][good][:, :, ~free].shape))
        assert not w["qd"][good][:, :, ~free].any() and w["clip_margin"].min() > 1e-9
    assert not res["all"]["err_max"].any() and not res["all"]["sat_steps"].any() and (res["all"]["steps"] > 0).all()
    lk, q, qd, qdd = tg.locked_inputs(c, "moving_nan")
    j = c["jl"]
    assert np.isnan(q[:, :, j]).any() and np.isnan(qd[:, :, j]).any() and np.isnan(qdd[:, :, j]).any() and np.isfinite(q[:, 0, j]).all()
    fq, fqd, fqdd = c["q"].copy(), c["qd"].copy(), c["qdd"].copy()
    fq[:, :, j], fqd[:, :, j], fqdd[:, :, j] = fq[:, :1, j], 0.0, 0.0
    flat = tg.locked_restatement(c, lk, fq, fqd, fqdd)
    for k in ("q", "qd", "t", "err_max", "err_end", "sat_steps", "steps", "status"):
        assert np.array_equal(res["moving_nan"][k], flat[k]), k
    clean = tg.locked_restatement(c, lk, c["q"], c["qd"], c["qdd"])
    keep = np.arange(tg.B) != 1
    for k in ("q", "qd", "err_max", "sat_steps"):
        assert np.array_equal(res["first_nan"][k][keep], clean[k][keep]), k


def test_the_clock_edges_in_the_restatement():
    """ceil((duration + settle) / dt) of tests/test_gpu_forward.test_the_clock_edges is exact at dt = 2^-9: 8 periods exactly,
    none at all, and GTO_TRACK_MAX_STEPS + 1 of them."""
    import test_gpu_forward as tg
    c = tg.clock_case()
    assert tg.MAX_STEPS == fr.MAX_STEPS and np.ceil(c["dur"] / tg.CLOCK_DT).tolist() == [8, 4, 6, 10] and c["dur"][0] / tg.CLOCK_DT == 8.0
    edge = c["dur"].copy()
    edge[1], edge[3] = 0.0, (tg.MAX_STEPS + 0.5) * tg.CLOCK_DT
    assert np.ceil(edge[3] / tg.CLOCK_DT) == tg.MAX_STEPS + 1
    w = tg.clock_restatement(c, edge)
    assert w["status"].tolist() == [0, 2, 0, 2] and w["steps"].tolist() == [8, 0, 6, 0] and np.isnan(w["q"][[1, 3]]).all()
    just = tg.clock_restatement(dict(c, q=c["q"][:1], qd=c["qd"][:1], qdd=c["qdd"][:1], model=tuple(a if a is None else a[:1] for a in c["model"]),
                                     plant=tuple(a if a is None else a[:1] for a in c["plant"])), np.array([0.0]))
    assert just["status"].tolist() == [2]


def test_exported_symbols_and_bindings():
    from grasptrajopt_amd import _capi, utils
    from grasptrajopt_amd.grasp_chain import GraspChain
    from grasptrajopt_amd.gto_planner import GTOPlanner
    for sym, n in (("gto_forward_dynamics", 12), ("gto_track_rollout", 29), ("gto_track_rollout_device", 30)):
        assert sym in _capi.EXPORTED_SYMBOLS and len(_capi.PROTOTYPES[sym][1]) == n
    for m in ("forward_dynamics", "track_rollout", "track_rollout_device"):
        assert callable(getattr(_capi.SolverHandle, m))
    assert list(inspect.signature(utils.forward_dynamics).parameters) == ["robot", "q", "qd", "tau", "payload", "link_ee", "locked"]
    sig = inspect.signature(utils.track_trajectories)
    assert list(sig.parameters) == ["robot", "retimed", "kp", "kd", "tau_max", "dt", "settle", "n_samples", "feedforward",
                                    "model_payload", "plant_payload", "locked", "link_ee"]
    assert [sig.parameters[k].default for k in ("tau_max", "dt", "settle", "n_samples", "feedforward")] == [None, 1e-3, 0.0, 100, "full"]
    assert "track" in inspect.signature(GTOPlanner.retrieve_path).parameters
    assert "track" in inspect.signature(GraspChain.plan_objects).parameters
    desc = dc.robot("panda")[0]
    kp, kd, tm, dt, settle, Mo, ff, lk = _capi.track_controller(desc, 100.0, KD)
    assert kp.tolist() == [100.0] * 9 and np.array_equal(kd, KD) and np.array_equal(tm, desc.effort)
    assert (dt, settle, Mo, ff, lk) == (1e-3, 0.0, 100, 2, None)
    lk = _capi.track_controller(desc, 1, 1, feedforward="none", locked=[0, 0, 1, 0, 0, 0, 0, 2, 0])
    assert lk[6] == 0 and lk[7].dtype == np.int32 and lk[7].tolist() == [0, 0, 1, 0, 0, 0, 0, 1, 0]
    for bad in (dict(kp=-1.0), dict(kp=np.nan), dict(kd=np.inf), dict(kp=[1, 2]), dict(tau_max=0.0), dict(tau_max=[np.nan] * 9),
                dict(dt=0.0), dict(dt=np.inf), dict(settle=-1e-3), dict(settle=np.nan), dict(n_samples=1), dict(feedforward=3),
                dict(feedforward="all"), dict(feedforward=True), dict(locked=[1, 0])):
        kw = dict(kp=1.0, kd=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            _capi.track_controller(desc, **kw)
    from grasptrajopt_amd.robot_desc import load_builtin
    with pytest.raises(ValueError, match="link inertials"):
        _capi.track_controller(load_builtin("panda"), 1.0, 1.0, tau_max=10.0)
