"""gto_forward_dynamics, gto_track_rollout and gto_track_rollout_device (csrc/gto_forward.h: fd_solve, k_forward_dynamics,
k_track_rollout) against tests/forward_ref.py, which tests/test_forward_cpu.py holds against physics, and the Python layers
above them.

Forward dynamics: the 11 robots of tests/dynamics_cases.py at n = 67 rows (more than one workgroup on every robot: a
workgroup holds fd_rows(F, ndof) = min(64, 63488 // ((15 F + ndof^2 + 7 ndof) 8 + 4)) rows) and n = 1; payload absent, mass
only, full; locked NULL, none, all but one, all.  Where `locked` leaves a joint free that moves no mass (the seeded robots
have a massless frame each) the case locks that joint too; the massless free joint has a test of its own.

Rollout: Panda, Fetch, prismatic_chain, limit_chain (32 frames, 16 free joints under locked = NULL: 18 passes in three
rounds of the 8 lanes a path gets there) and four of the smallest robots (root_joint, chain_1, prismatic_only,
ee_above_joints: four paths of 16 lanes share a workgroup there, ROLLOUT_LAYOUTS), B = 5, M = 9, Mo = 7, dt = 2 ms, at most 30 steps (5 on limit_chain, whose numpy
restatement takes a quarter of a second per step), every feedforward mode, the plant's payload not the model's, one case that saturates.
Tolerance of q_out, qd_out, err_max, err_end: 16 d, d the largest difference between the restatement run with its two
mass-matrix orderings (Jacobian sum / unit-acceleration columns) over these very cases, measured on the CPU with
forward_ref.rollout_batch(columns=False) against (columns=True); the GPU's frame-local arithmetic is a third ordering of the
same sums, and the factor covers its contraction into FMAs.  Measured, the largest over the four modes of each robot:
    panda 4.33e-15   fetch 5.67e-12   prismatic_chain 1.57e-12   limit_chain 1.44e-11
    root_joint 6.61e-15   chain_1 6.16e-14   prismatic_only 4.72e-16   ee_above_joints 3.49e-11
so d = ROLLOUT_D = 3.49e-11 (the seeded bodies of the generated robots make worse-conditioned mass matrices than Panda's).
The clock's edges (Panda, dt = 2^-9 s): 3.72e-15, under ROLLOUT_D.  The locked settings have a d per robot, LOCKED_D, measured
the same way over the five settings: panda 5.60e-13, chain_1 8.78e-15, limit_chain 6.10e-10 (all 31 joints free under a
reference that asks for 1000 rad/s^2: every step saturates and err_max reaches 0.34 rad in three steps).
The same for the energy drifts of the free fall at h = 0.02 and 0.01: 2.84e-14 and 1.42e-14, ENERGY_D = 2.84e-14 (one unit
of round-off of an energy of 103 J is 2.3e-14).
No case's own | |tau| - tau_max | comes within 1e-9 relative of a clip decision: the smallest margin over all of them is
4.4e-3 (measured there, asserted here again on the restatement's run), so sat_steps and steps must be equal.
"""
import ctypes as C
import os

import numpy as np
import pytest

import dynamics_cases as dc
import dynamics_ref as dr
import forward_ref as fr
from test_dynamics_cpu import mass_matrix

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 67
ROLLOUT_ROBOTS = ("panda", "fetch", "prismatic_chain", "limit_chain", "root_joint", "chain_1", "prismatic_only", "ee_above_joints")
LOCKED_ROBOTS = ("panda", "chain_1", "limit_chain")
# (G lanes per path, P paths per workgroup) of k_track_rollout, as track_layout restates them
ROLLOUT_LAYOUTS = {"panda": (16, 2), "fetch": (16, 2), "prismatic_chain": (16, 3), "limit_chain": (8, 1), "root_joint": (16, 4),
                   "chain_1": (16, 4), "prismatic_only": (16, 4), "ee_above_joints": (16, 4)}
ROLLOUT_D = 3.49e-11
ENERGY_D = 2.84e-14
B, M, MO, DT = 5, 9, 7, 2e-3


def same(a, b):
    """Bit for bit; a NaN equals a NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float64:
        return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def fd_rows(F, ndof):
    """fd_rows_per_block of csrc/gto_forward.h, restated from its constants."""
    return min(64, (64 * 1024 - 2048) // ((15 * F + ndof * ndof + 7 * ndof) * 8 + 4))


def track_layout(F, ndof):
    """(G, P) of k_track_rollout: track_group_lanes and track_paths_per_block of csrc/gto_forward.h, restated from its
    constants (15 rt_rnea slots per frame and lane, 15 work vectors and four ints per path, 64 KB less 2048 bytes)."""
    room = 64 * 1024 - 2048
    path = lambda G: (15 * F * G + ndof * ndof + 15 * ndof) * 8 + 16  # noqa: E731
    G = 16
    while G > 1 and path(G) > room:
        G //= 2
    return G, min(room // path(G), 64 // G)


def as_dict(pl, rows=slice(None)):
    if pl is None:
        return None
    return {k: v[rows] for k, v in zip(("mass", "com", "inertia"), pl) if v is not None}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


# ------------------------------------------------------------------------------------------------ forward dynamics
@pytest.fixture(scope="module", params=dc.NAMES)
def case(request, capi):
    desc, ee, gr, ngp = dc.robot(request.param)
    h = capi.SolverHandle(desc, ee, gr, device=0, n_gripper_points=ngp)
    q, qd, _ = dr.in_limit_states(desc, N, seed=31)
    qd[62:] = 0.0  # rows at rest
    tau = np.random.default_rng(32).uniform(-15.0, 15.0, q.shape)
    pls = dc.payloads(N, seed=33)
    eef = desc.frame_index(ee)
    ref = {}  # the mass matrix (Jacobian sum) and the bias of every row, once per payload kind
    for kind, pl in pls.items():
        Ms, cs = [], []
        for i in range(N):
            p = None if pl is None else (pl[0][i], None if pl[1] is None else pl[1][i], None if pl[2] is None else pl[2][i])
            Ms.append(mass_matrix(desc, q[i], eef, p))
            cs.append(dr.inverse_dynamics(desc, q[i], qd[i], np.zeros(desc.ndof), eef, p))
        ref[kind] = (np.stack(Ms), np.stack(cs))
    named = fr.named_joints(desc)
    moving = named & (np.diag(ref["none"][0][0]) > 0)
    one = np.ones(desc.ndof, dtype=np.int32)
    if moving.any():
        one[np.flatnonzero(moving)[0]] = 0
    massless_opt = fr.free_joints(desc) & ~moving
    locked = {"null": None if not massless_opt.any() else (~(fr.free_joints(desc) & moving)).astype(np.int32),
              "none": (~moving).astype(np.int32), "all_but_one": one, "all": np.ones(desc.ndof, dtype=np.int32)}
    yield dict(name=request.param, desc=desc, h=h, ee=eef, q=q, qd=qd, tau=tau, payloads=pls, ref=ref, locked=locked, named=named,
               moving=moving, null_is_default=not massless_opt.any())
    h.close()


def test_the_robots_cover_the_layouts():
    shapes = {name: (dc.robot(name)[0].n_frames, dc.robot(name)[0].ndof) for name in dc.NAMES}
    rows = {fd_rows(*s) for s in shapes.values()}
    assert 64 in rows and min(rows) <= 4 and all(r < N for r in rows)  # more than one workgroup on every robot


@pytest.mark.parametrize("kind", ["none", "mass", "full"])
def test_forward_dynamics_matches_the_reference(case, kind):
    d, h, pl = case["desc"], case["h"], case["payloads"][kind]
    Mref, cref = case["ref"][kind]
    q, qd, tau = case["q"], case["qd"], case["tau"]
    rows = fd_rows(d.n_frames, d.ndof)
    assert case["null_is_default"] or case["name"] not in ("panda", "fetch")  # locked = NULL itself runs on the real robots
    for lname, locked in case["locked"].items():
        qdd, status, Mout = h.forward_dynamics(q, qd, tau, as_dict(pl), locked, want_mass_matrix=True)
        free = fr.free_joints(d, locked)
        assert (status == 0).all() and np.isfinite(qdd).all() and (qdd[:, ~free] == 0).all(), (lname, status)
        if lname == "all":
            assert not free.any() and not qdd.any()
        assert np.array_equal(Mout, Mout.transpose(0, 2, 1))  # exactly symmetric
        assert not Mout[:, ~case["named"], :].any() and not Mout[:, :, ~case["named"]].any()
        scaleM = np.abs(Mref).max(axis=(1, 2))
        errM = np.abs(Mout - Mref).max(axis=(1, 2)) / scaleM
        worst_rt = worst_q = 0.0
        for i in range(N):
            p = None if pl is None else (pl[0][i], None if pl[1] is None else pl[1][i], None if pl[2] is None else pl[2][i])
            if free.any():
                Mff = Mref[i][np.ix_(free, free)]
                want = np.linalg.solve(Mff, (tau[i] - cref[i])[free])
                tol = 1e-11 * np.linalg.cond(Mff) * max(1.0, np.abs(want).max())
                worst_q = max(worst_q, np.abs(qdd[i, free] - want).max() / tol)
                back = dr.inverse_dynamics(d, q[i], qd[i], qdd[i], case["ee"], p)
                scale = max(1.0, np.abs(tau[i]).max(), (np.abs(Mref[i]) @ np.abs(qdd[i])).max())
                worst_rt = max(worst_rt, np.abs(back - tau[i])[free].max() / scale)
        print(f"{case['name']} {kind} locked={lname}: round trip {worst_rt:.2e}, qdd error / tolerance {worst_q:.2e}, M {errM.max():.2e}")
        assert worst_rt <= 1e-11 and worst_q <= 1.0 and errM.max() <= 1e-11
        for i in (0, min(rows, N - 2), N - 1):  # a row alone is the row inside the batch, bit for bit
            a, s, Ma = h.forward_dynamics(q[i], qd[i], tau[i], as_dict(pl, slice(i, i + 1)), locked, want_mass_matrix=True)
            assert same(a[0], qdd[i]) and s[0] == 0 and same(Ma[0], Mout[i]), (lname, i)


def test_rows_that_fail_fail_alone(case):
    d, h = case["desc"], case["h"]
    q, qd, tau = case["q"].copy(), case["qd"].copy(), case["tau"].copy()
    locked = case["locked"]["none"]
    good, s0, M0 = h.forward_dynamics(q, qd, tau, None, locked, want_mass_matrix=True)
    q[3, 0], qd[40, d.ndof - 1], tau[N - 1, 0] = np.nan, np.inf, np.nan
    got, s, Mg = h.forward_dynamics(q, qd, tau, None, locked, want_mass_matrix=True)
    bad = np.zeros(N, dtype=bool)
    bad[[3, 40, N - 1]] = True
    assert (s[bad] == 2).all() and (s[~bad] == 0).all()
    assert np.isnan(got[bad]).all() and np.isnan(Mg[bad]).all() and same(got[~bad], good[~bad]) and same(Mg[~bad], M0[~bad])
    massless = case["named"] & ~case["moving"]
    if massless.any():  # freed, the joint that moves no mass is a pivot of 0: every row, and nothing else is touched
        got, s = h.forward_dynamics(case["q"], case["qd"], case["tau"], None, np.zeros(d.ndof, dtype=np.int32))
        assert (s == 2).all() and np.isnan(got).all()


def test_a_massless_finger_is_numerical_alone(capi):
    desc, ee, gr, _ = dc.robot("panda")
    h = capi.SolverHandle(desc, ee, gr, device=0)
    q, qd, _ = dr.in_limit_states(desc, 4, seed=34)
    tau = np.ones_like(q)
    none = np.zeros(desc.ndof, dtype=np.int32)
    good = h.forward_dynamics(q, qd, tau, None, none)
    assert (good[1] == 0).all()
    mass = desc.frame_mass.copy()
    mass[desc.frame_index("panda_rightfinger")] = 0.0
    try:
        h.set_link_inertials(mass, desc.frame_com, desc.frame_inertia)
        qdd, s = h.forward_dynamics(q, qd, tau, None, none)
        assert (s == 2).all() and np.isnan(qdd).all()
        qdd, s = h.forward_dynamics(q, qd, tau)  # the fingers locked: the arm does not care
        assert (s == 0).all() and np.isfinite(qdd).all()
    finally:
        h.set_link_inertials(desc.frame_mass, desc.frame_com, desc.frame_inertia)
    assert same(h.forward_dynamics(q, qd, tau, None, none)[0], good[0])
    h.close()


def test_refusals_leave_the_handle_and_the_outputs_alone(capi):
    from grasptrajopt_amd.robot_desc import load_builtin
    desc, ee, gr, _ = dc.robot("panda")
    h = capi.SolverHandle(load_builtin("panda"), ee, gr, device=0)
    nd = desc.ndof
    q = np.zeros((2, nd))
    with pytest.raises(capi.GTOError, match=r"\(-1\): no link inertials set$"):
        h.forward_dynamics(q, q, q)
    with pytest.raises(capi.GTOError, match=r"\(-1\): no link inertials set$"):
        h.track_rollout(np.ones(2), np.zeros((2, 3, nd)), np.zeros((2, 3, nd)), np.zeros((2, 3, nd)), 1.0, 1.0, tau_max=10.0)
    h.set_link_inertials(desc.frame_mass, desc.frame_com, desc.frame_inertia)
    good = h.forward_dynamics(q, q, q)[0]
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    p = lambda a: None if a is None else a.ctypes.data_as(pd if a.dtype == np.float64 else pi)  # noqa: E731
    out, st = np.full((2, nd), 7.0), np.full(2, 7, dtype=np.int32)
    lib = h.lib
    for mass, com, why in ((np.array([1.0, -0.5]), None, "payload mass must be >= 0 and finite"),
                           (np.array([np.nan, 1.0]), None, "payload mass must be >= 0 and finite"),
                           (None, np.zeros((2, 3)), "payload_com / payload_inertia without payload_mass")):
        rc = lib.gto_forward_dynamics(h._h, 2, p(q), p(q), p(q), p(mass), p(com), None, None, p(out), None, p(st))
        assert rc == -1 and lib.gto_last_error(h._h).decode() == why and (out == 7.0).all() and (st == 7).all()
    assert lib.gto_forward_dynamics(h._h, 2, p(q), None, p(q), None, None, None, None, p(out), None, None) == -1
    assert lib.gto_forward_dynamics(h._h, -1, p(q), p(q), p(q), None, None, None, None, p(out), None, None) == -1
    assert lib.gto_forward_dynamics(h._h, 0, None, None, None, None, None, None, None, None, None, None) == 0
    # the rollout's host arrays and scalars
    ref = np.zeros((2, 3, nd))
    dur, one, eff = np.ones(2), np.ones(nd), np.full(nd, 50.0)

    def roll(kp=one, kd=one, tm=eff, dt=1e-3, settle=0.0, ff=2, M=3, Mo=4, mm=None, mc=None, pm=None, dur_=dur):
        return lib.gto_track_rollout(h._h, 2, M, p(dur_), p(ref), p(ref), p(ref), p(kp), p(kd), p(tm), dt, settle, ff, p(mm), p(mc), None,
                                     p(pm), None, None, None, Mo, p(out), None, None, None, None, None, None, p(st))

    neg, nan, zero = one.copy(), one.copy(), eff.copy()
    neg[2], nan[nd - 1], zero[0] = -1.0, np.nan, 0.0
    for kw, why in ((dict(kp=neg), "kp and kd must be finite and >= 0"), (dict(kd=nan), "kp and kd must be finite and >= 0"),
                    (dict(kp=np.full(nd, np.inf)), "kp and kd must be finite and >= 0"),
                    (dict(tm=zero), "tau_max must be > 0 (+inf: no limit)"), (dict(tm=nan), "tau_max must be > 0 (+inf: no limit)"),
                    (dict(dt=0.0), "dt must be finite and > 0"), (dict(dt=np.inf), "dt must be finite and > 0"),
                    (dict(settle=-1.0), "settle must be finite and >= 0"), (dict(settle=np.nan), "settle must be finite and >= 0"),
                    (dict(ff=3), "feedforward must be 0, 1 or 2"), (dict(ff=-1), "feedforward must be 0, 1 or 2"),
                    (dict(M=1), "M and Mo must be >= 2"), (dict(Mo=1), "M and Mo must be >= 2"),
                    (dict(mm=np.array([1.0, -1.0])), "payload mass must be >= 0 and finite"),
                    (dict(pm=np.array([np.inf, 1.0])), "payload mass must be >= 0 and finite"),
                    (dict(mc=np.zeros((2, 3))), "payload_com / payload_inertia without payload_mass"),
                    (dict(dur_=None), "null reference array")):
        assert roll(**kw) == -1 and lib.gto_last_error(h._h).decode() == "gto_track_rollout: " + why, kw
        assert (out == 7.0).all() and (st == 7).all()
    assert same(h.forward_dynamics(q, q, q)[0], good)
    h.close()


@pytest.mark.parametrize("name", ["panda", "fetch"])
def test_utils_forward_dynamics_is_the_abi_call(name, capi):
    from grasptrajopt_amd import utils
    from grasptrajopt_amd.gto_models import GTORobotModel
    from grasptrajopt_amd.robot_desc import load_builtin
    d, ee, gr, _ = dc.robot(name)
    h = capi.SolverHandle(d, ee, gr, device=0)
    q, qd, tau = dr.in_limit_states(d, 9, seed=35)
    robot = GTORobotModel(desc=d, device=0)
    pl = as_dict(dc.payloads(9, seed=36)["full"])
    assert same(utils.forward_dynamics(robot, q, qd, tau, payload=pl, link_ee=ee), h.forward_dynamics(q, qd, tau, pl)[0])
    lk = np.zeros(d.ndof, dtype=np.int32)
    lk[1] = 1
    assert same(utils.forward_dynamics(robot, q, qd, tau, locked=lk), h.forward_dynamics(q, qd, tau, None, lk)[0])
    one = utils.forward_dynamics(robot, q[3], qd[3], tau[3])
    assert one.shape == (d.ndof,) and same(one, h.forward_dynamics(q[3], qd[3], tau[3])[0][0])
    with pytest.raises(ValueError, match="needs link_ee"):
        utils.forward_dynamics(robot, q[3], qd[3], tau[3], payload={"mass": 1.0})
    bare = GTORobotModel(desc=load_builtin(name), device=0)
    with pytest.raises(ValueError, match="no link inertials"):
        utils.forward_dynamics(bare, q, qd, tau)
    h.close()
    for hh in robot._handles.values():
        hh.close()


# ------------------------------------------------------------------------------------------------ the rollout
# durations of the five paths as multiples of the robot's longest (30 steps of 2 ms with the settle time); the fourth path
# carries a NaN
DURATIONS = np.array([0.05, 0.024, 0.0, 0.03, 0.013])
SCALE = {"limit_chain": 0.1}
SETTLE = {"limit_chain": 0.004}  # 5 steps; 2 on the slow one
MODES = ("none", "gravity", "full", "saturating")


def rollout_case(name, free=None, scale=None):
    """The inputs of the rollout cases of one robot: seeded smooth references from an in-limit start, gains, limits, payloads.
    free: the joints that move and are controlled (None: the ones locked = NULL leaves free); scale: of DURATIONS (None:
    the robot's SCALE)."""
    desc, ee, gr, ngp = dc.robot(name)
    rng = np.random.default_rng(41)
    free = fr.free_joints(desc) if free is None else free
    q0, _, _ = dr.in_limit_states(desc, B, seed=42)
    dur = DURATIONS * (SCALE.get(name, 1.0) if scale is None else scale)
    amp = np.where(free, rng.uniform(-0.005, 0.005, (B, desc.ndof)), 0.0)
    T = np.maximum(dur, 1e-3)[:, None, None]
    x = np.linspace(0.0, 1.0, M)[None, :, None]
    s, sd, sdd = 0.5 * (1 - np.cos(np.pi * x)), 0.5 * np.pi * np.sin(np.pi * x) / T, 0.5 * np.pi ** 2 * np.cos(np.pi * x) / T ** 2
    q = q0[:, None, :] + amp[:, None, :] * s
    qd, qdd = amp[:, None, :] * sd, amp[:, None, :] * sdd
    eef = desc.frame_index(ee)
    g = np.abs(np.stack([dr.inverse_dynamics(desc, q0[b], 0 * q0[b], 0 * q0[b], eef) for b in range(B)])).max(axis=0)
    tau_max = np.where(free, 3.0 * np.maximum(g, 1.0) + 20.0, np.inf)
    j = int(np.flatnonzero(free)[np.argmax(g[free])])
    weak = tau_max.copy()
    weak[j] = 0.4 * np.abs(dr.inverse_dynamics(desc, q0[0], 0 * q0[0], 0 * q0[0], eef))[j] + 1e-3  # path 0 cannot hold there
    kp, kd = np.where(free, 200.0, 0.0), np.where(free, 10.0, 0.0)
    model = dc.payloads(B, seed=43)["mass"]
    plant = dc.payloads(B, seed=44)["full"]
    return dict(desc=desc, ee=ee, eef=eef, gr=gr, ngp=ngp, dur=dur, q=q, qd=qd, qdd=qdd, kp=kp, kd=kd, tau_max=tau_max, weak=weak,
                model=model, plant=plant, free=free, settle=SETTLE.get(name, 0.01))


def mode_args(c, mode):
    return dict(feedforward={"none": 0, "gravity": 1, "full": 2, "saturating": 2}[mode], tau_max=c["weak"] if mode == "saturating" else c["tau_max"])


def with_nan(c):
    q = c["q"].copy()
    q[3, M // 2, int(np.flatnonzero(c["free"])[0])] = np.nan
    return q


def gpu_rollout(h, c, mode, q=None, rows=slice(None), n_samples=MO):
    a = mode_args(c, mode)
    return h.track_rollout(c["dur"][rows], (c["q"] if q is None else q)[rows], c["qd"][rows], c["qdd"][rows], c["kp"], c["kd"],
                           tau_max=a["tau_max"], dt=DT, settle=c["settle"], n_samples=n_samples, feedforward=a["feedforward"],
                           model_payload=as_dict(c["model"], rows), plant_payload=as_dict(c["plant"], rows))


@pytest.fixture(scope="module", params=ROLLOUT_ROBOTS)
def roll(request, capi):
    c = rollout_case(request.param)
    c["name"] = request.param
    c["h"] = capi.SolverHandle(c["desc"], c["ee"], c["gr"], device=0, n_gripper_points=c["ngp"])
    yield c
    c["h"].close()


def test_the_rollout_robots_cover_the_layouts():
    """The three workgroup layouts of k_track_rollout: four paths of 16 lanes (all 64 lanes busy, the five paths fill one
    workgroup and leave a second with one valid group of four), two or three paths, and one path of 8 lanes."""
    layouts = {name: track_layout(dc.robot(name)[0].n_frames, dc.robot(name)[0].ndof) for name in ROLLOUT_ROBOTS}
    assert layouts == ROLLOUT_LAYOUTS
    seen = set(layouts.values())
    assert (16, 4) in seen and seen & {(16, 2), (16, 3)} and (8, 1) in seen
    assert all(layouts[name] == (16, 4) for name in ("root_joint", "chain_1", "prismatic_only", "ee_above_joints"))
    assert {layouts[name] for name in LOCKED_ROBOTS} == {(16, 2), (16, 4), (8, 1)}


@pytest.mark.parametrize("mode", MODES)
def test_rollout_matches_the_restatement(roll, mode):
    c, h = roll, roll["h"]
    a = mode_args(c, mode)
    qn = with_nan(c)
    want = fr.rollout_batch(c["desc"], c["eef"], c["dur"], qn, c["qd"], c["qdd"], c["kp"], c["kd"], a["tau_max"], dt=DT, settle=c["settle"],
                            n_samples=MO, feedforward=a["feedforward"], model_payload=c["model"], plant_payload=c["plant"])
    got = gpu_rollout(h, c, mode, qn)
    assert want["clip_margin"].min() > 1e-9  # no clip decision hangs on round-off
    assert want["status"].tolist() == [0, 0, 0, 2, 0] and got["status"].tolist() == [0, 0, 0, 2, 0]
    assert np.array_equal(got["steps"], want["steps"]) and np.array_equal(got["sat_steps"], want["sat_steps"])
    assert got["steps"].max() <= 60 and got["steps"][2] == round(c["settle"] / DT) and got["steps"][3] == 0 and got["sat_steps"][3] == 0
    if mode == "saturating":
        assert got["sat_steps"][0] > got["steps"][0] // 2
    assert same(got["t"], want["t"])
    tol = 16 * ROLLOUT_D
    err = {k: np.nanmax(np.abs(got[k] - want[k])) for k in ("q", "qd", "err_max", "err_end")}
    print(f"{c['name']} {mode}: steps {got['steps'].tolist()} sat {got['sat_steps'].tolist()} differences {err}, allowed {tol:.2e}")
    for k in ("q", "qd", "t", "err_max", "err_end"):
        assert np.isnan(got[k][3]).all() and np.isfinite(np.delete(got[k], 3, axis=0)).all()
    assert max(err.values()) <= tol
    # the NaN path's neighbours are bit for bit what they are without it
    clean = gpu_rollout(h, c, mode)
    for k in got:
        assert same(np.delete(got[k], 3, axis=0), np.delete(clean[k], 3, axis=0)), k
    assert clean["status"][3] == 0


def test_energy_drift_matches_the_restatement(capi):
    """The free fall of tests/test_forward_cpu.py's check 2 at h = 0.02 and 0.01."""
    desc, ee, gr, _ = dc.robot("panda")
    eef = desc.frame_index(ee)
    h = capi.SolverHandle(desc, ee, gr, device=0)
    q, qd, _ = dr.in_limit_states(desc, 1, seed=9)
    free = fr.free_joints(desc)
    q0, qd0 = q[0], np.where(free, 0.5 * qd[0], 0.0)
    E0 = fr.energy(desc, q0, qd0, eef)
    ref = np.stack([q0, q0])[None], np.stack([qd0, qd0])[None], np.zeros((1, 2, desc.ndof))
    for step in (0.02, 0.01):
        want = fr.rollout(desc, eef, 0.2, ref[0][0], ref[1][0], ref[2][0], 0.0, 0.0, np.inf, dt=step, n_samples=2, feedforward=0)
        got = h.track_rollout([0.2], *ref, 0.0, 0.0, tau_max=np.inf, dt=step, n_samples=2, feedforward="none")
        dw = fr.energy(desc, want["q"][1], want["qd"][1], eef) - E0
        dg = fr.energy(desc, got["q"][0, 1], got["qd"][0, 1], eef) - E0
        print(f"h = {step}: energy drift gpu {dg:.6e}, restatement {dw:.6e}")
        assert got["status"][0] == 0 and got["steps"][0] == want["steps"] and abs(dg - dw) <= 16 * ENERGY_D
    h.close()


def test_a_path_is_the_same_in_any_batch(roll):
    c, h = roll, roll["h"]
    five = gpu_rollout(h, c, "full")
    for b in range(B):
        alone = gpu_rollout(h, c, "full", rows=slice(b, b + 1))
        for k in five:
            assert same(alone[k][0], five[k][b]), (b, k)
    idx = np.arange(70) % B
    idx[[0, 69]] = [4, 1]
    c70 = dict(c, dur=c["dur"][idx], q=c["q"][idx], qd=c["qd"][idx], qdd=c["qdd"][idx],
               model=tuple(None if a is None else a[idx] for a in c["model"]), plant=tuple(None if a is None else a[idx] for a in c["plant"]))
    many = gpu_rollout(h, c70, "full")
    for k in five:
        assert same(many[k], five[k][idx]), k
    other = gpu_rollout(h, c, "full", n_samples=12)  # more samples than some paths have steps: repeated states, the same numbers
    for k in ("err_max", "err_end", "sat_steps", "steps", "status"):
        assert same(other[k], five[k])
    assert same(other["q"][:, -1], five["q"][:, -1]) and same(other["q"][:, 0], c["q"][:, 0])


def device_rollout(h, c, mode, tensors, stream, dt=DT, settle=None, locked=None):
    import torch
    a = mode_args(c, mode)
    nb = tensors["dur"].shape[0]
    out = dict(q=torch.full((nb, MO, c["desc"].ndof), 7.0, dtype=torch.float64, device="cuda:0"),
               qd=torch.full((nb, MO, c["desc"].ndof), 7.0, dtype=torch.float64, device="cuda:0"),
               t=torch.full((nb, MO), 7.0, dtype=torch.float64, device="cuda:0"),
               err_max=torch.full((nb,), 7.0, dtype=torch.float64, device="cuda:0"),
               err_end=torch.full((nb,), 7.0, dtype=torch.float64, device="cuda:0"),
               sat_steps=torch.full((nb,), 7, dtype=torch.int32, device="cuda:0"), steps=torch.full((nb,), 7, dtype=torch.int32, device="cuda:0"),
               status=torch.full((nb,), 7, dtype=torch.int32, device="cuda:0"))
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    h.track_rollout_device(nb, M, ptr(tensors["dur"]), ptr(tensors["q"]), ptr(tensors["qd"]), ptr(tensors["qdd"]), c["kp"], c["kd"],
                           tau_max=a["tau_max"], dt=dt, settle=c["settle"] if settle is None else settle, n_samples=MO,
                           feedforward=a["feedforward"], model_payload=[ptr(x) for x in tensors["model"]],
                           plant_payload=[ptr(x) for x in tensors["plant"]], locked=locked,
                           q_out=ptr(out["q"]), qd_out=ptr(out["qd"]), t_out=ptr(out["t"]), err_max=ptr(out["err_max"]),
                           err_end=ptr(out["err_end"]), sat_steps=ptr(out["sat_steps"]), steps=ptr(out["steps"]),
                           status_out=ptr(out["status"]), stream=stream.cuda_stream)
    return out


def to_device(c, q):
    import torch
    cu = lambda a: None if a is None else torch.from_numpy(np.array(a, order="C")).to("cuda:0")  # noqa: E731
    return dict(dur=cu(c["dur"]), q=cu(q), qd=cu(c["qd"]), qdd=cu(c["qdd"]), model=[cu(a) for a in c["model"]],
                plant=[cu(a) for a in c["plant"]])


def test_device_variant_equals_the_host_variant_and_keeps_stream_order(roll):
    import time
    import torch
    import held_stream as hs
    c, h = roll, roll["h"]
    qn = with_nan(c)
    want = gpu_rollout(h, c, "saturating", qn)
    stream = torch.cuda.Stream(device="cuda:0")
    with hs.Scenario() as sc:
        true = sc.keep(to_device(c, qn))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sc.keep(device_rollout(h, c, "saturating", true, stream))
        t_host = time.perf_counter() - t0
        stream.synchronize()
        for k in want:
            assert same(out[k].cpu().numpy(), want[k]), k
        # behind a busy stream: the inputs arrive on the stream after the hold, the call must not run ahead of them
        blank = lambda x: None if x is None else torch.zeros_like(x)  # noqa: E731
        late = sc.keep({k: ([blank(x) for x in v] if isinstance(v, list) else blank(v)) for k, v in true.items()})
        event = hs.hold(stream, hs.hold_ms(t_host))
        with torch.cuda.stream(stream):
            for k, v in true.items():
                for dst, src in zip(late[k] if isinstance(v, list) else [late[k]], v if isinstance(v, list) else [v]):
                    if src is not None:
                        dst.copy_(src, non_blocking=True)
        out2 = sc.keep(device_rollout(h, c, "saturating", late, stream))
        returned_while_held = hs.still_held(event)
        stream.synchronize()
        print(f"{c['name']}: returned while the stream was held: {returned_while_held}, enqueue {1e3 * t_host:.3f} ms")
        for k in want:
            assert same(out2[k].cpu().numpy(), want[k]), k
        assert returned_while_held  # no synchronisation inside the call


# ------------------------------------------------------------------------------------------------ locked joints
LOCKED_SETTINGS = ("none", "all_but_one", "all", "moving_nan", "first_nan")
# (scale of DURATIONS, settle time): at most 8 steps on Panda, whose restatement with nine free joints takes 80 ms per step,
# and at most 3 on limit_chain, where 31 joints are free (33 passes over 8 lanes)
LOCKED_CLOCK = {"panda": (0.2, 0.004), "chain_1": (1.0, 0.01), "limit_chain": (0.1, 0.0009)}
LOCKED_MAX_STEPS = {"panda": 8, "chain_1": 30, "limit_chain": 3}
# d of these cases, measured as ROLLOUT_D is (the largest over the five settings of a robot; the head of the file)
LOCKED_D = {"panda": 5.60e-13, "chain_1": 8.78e-15, "limit_chain": 6.10e-10}


def locked_case(name):
    """rollout_case with every named joint moving in the reference and under control, gains and limits that differ from
    joint to joint, and what the `locked` settings need: moving (the joints that move mass at the start state), jl (a
    joint locked = NULL leaves free, the middle one of them: the settings moving_nan and first_nan lock it too)."""
    desc = dc.robot(name)[0]
    named = fr.named_joints(desc)
    c = rollout_case(name, free=named, scale=LOCKED_CLOCK[name][0])
    c["settle"] = LOCKED_CLOCK[name][1]
    rng = np.random.default_rng(45)
    c["kp"], c["kd"] = np.where(named, rng.uniform(100.0, 300.0, desc.ndof), 0.0), np.where(named, rng.uniform(5.0, 15.0, desc.ndof), 0.0)
    c["tau_max"] = c["tau_max"] * rng.uniform(1.0, 1.5, desc.ndof)
    c["moving"] = named & (np.diag(mass_matrix(desc, c["q"][0, 0], c["eef"], None)) > 0)
    default = np.flatnonzero(fr.free_joints(desc))
    c["jl"] = int(default[len(default) // 2])
    return c


def locked_inputs(c, setting):
    """(locked (ndof,) int32, q, qd, qdd) of a setting."""
    nd = c["desc"].ndof
    q, qd, qdd = c["q"].copy(), c["qd"].copy(), c["qdd"].copy()
    if setting == "none":  # massless joints excepted: freed, they are a pivot of 0
        lk = ~c["moving"]
    elif setting == "all_but_one":
        lk = np.ones(nd, dtype=bool)
        lk[np.flatnonzero(c["moving"])[c["moving"].sum() // 2]] = False
    elif setting == "all":
        lk = np.ones(nd, dtype=bool)
    else:
        lk = ~fr.free_joints(c["desc"])
        j = c["jl"]
        lk[j] = True
        assert (np.abs(q[:, -1, j] - q[:, 0, j]) > 1e-4).all()  # its reference moves, on the path of duration 0 too
        if setting == "moving_nan":  # whatever the reference says about a locked joint past its first position is ignored
            q[0, 1, j] = qd[0, 0, j] = qdd[0, M - 1, j] = q[1, M - 1, j] = qd[4, M // 2, j] = np.nan
        else:
            q[1, 0, j] = np.nan
    return lk.astype(np.int32), q, qd, qdd


@pytest.fixture(scope="module", params=LOCKED_ROBOTS)
def lock(request, capi):
    c = locked_case(request.param)
    c["name"] = request.param
    c["h"] = capi.SolverHandle(c["desc"], c["ee"], c["gr"], device=0, n_gripper_points=c["ngp"])
    yield c
    c["h"].close()


def locked_rollout(h, c, lk, q, qd, qdd):
    return h.track_rollout(c["dur"], q, qd, qdd, c["kp"], c["kd"], tau_max=c["tau_max"], dt=DT, settle=c["settle"], n_samples=MO,
                           feedforward=2, model_payload=as_dict(c["model"]), plant_payload=as_dict(c["plant"]), locked=lk)


def locked_restatement(c, lk, q, qd, qdd, **kw):
    return fr.rollout_batch(c["desc"], c["eef"], c["dur"], q, qd, qdd, c["kp"], c["kd"], c["tau_max"], dt=DT, settle=c["settle"],
                            n_samples=MO, feedforward=2, model_payload=c["model"], plant_payload=c["plant"], locked=lk, **kw)


@pytest.mark.parametrize("setting", LOCKED_SETTINGS)
def test_rollout_with_locked_joints(lock, setting):
    """The rollout's `locked` argument with other lists than the default, each against forward_ref.rollout_batch(locked=...)
    at 16 d, d = LOCKED_D of the robot."""
    c, h = lock, lock["h"]
    tol = 16 * LOCKED_D[c["name"]]
    lk, q, qd, qdd = locked_inputs(c, setting)
    free = fr.free_joints(c["desc"], lk)
    want = locked_restatement(c, lk, q, qd, qdd)
    got = locked_rollout(h, c, lk, q, qd, qdd)
    bad = np.zeros(B, dtype=bool)
    bad[1] = setting == "first_nan"
    assert want["clip_margin"].min() > 1e-9
    assert np.array_equal(want["status"], np.where(bad, 2, 0)) and np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["steps"], want["steps"]) and np.array_equal(got["sat_steps"], want["sat_steps"])
    assert got["steps"].max() <= LOCKED_MAX_STEPS[c["name"]] and same(got["t"], want["t"])
    err = {k: np.abs(got[k][~bad] - want[k][~bad]).max() for k in ("q", "qd", "err_max", "err_end")}
    print(f"{c['name']} locked {setting}: {int(free.sum())} free, steps {got['steps'].tolist()} differences {err}, allowed {tol:.2e}")
    for k in ("q", "qd", "t", "err_max", "err_end"):
        assert np.isnan(got[k][bad]).all() and np.isfinite(got[k][~bad]).all()
    assert max(err.values()) <= tol
    # a locked joint stands at its first position with no velocity, whatever its reference does
    assert same(got["q"][~bad][:, :, ~free], np.broadcast_to(q[~bad][:, :1, ~free], got["q"][~bad][:, :, ~free].shape))
    assert not got["qd"][~bad][:, :, ~free].any()
    if setting == "none":
        assert free.sum() == c["moving"].sum() and (c["name"] != "limit_chain" or free.sum() == 31)
    if setting == "all":
        assert not free.any() and same(got["q"], np.broadcast_to(q[:, :1], got["q"].shape)) and not got["qd"].any()
        assert not got["err_max"].any() and not got["err_end"].any() and not got["sat_steps"].any() and (got["steps"] > 0).all()
    if setting == "moving_nan":  # bit for bit the run with that joint's reference flattened
        j = c["jl"]
        fq, fqd, fqdd = c["q"].copy(), c["qd"].copy(), c["qdd"].copy()
        fq[:, :, j], fqd[:, :, j], fqdd[:, :, j] = fq[:, :1, j], 0.0, 0.0
        flat = locked_rollout(h, c, lk, fq, fqd, fqdd)
        for k in got:
            assert same(got[k], flat[k]), k
    if setting == "first_nan":  # the neighbours are what they are without it
        clean = locked_rollout(h, c, lk, c["q"], c["qd"], c["qdd"])
        assert (clean["status"] == 0).all()
        for k in got:
            assert same(got[k][~bad], clean[k][~bad]), k


# ------------------------------------------------------------------------------------------------ the clock's edges
MAX_STEPS = 1 << 20  # GTO_TRACK_MAX_STEPS
CLOCK_DT = 2.0 ** -9  # a power of two: (duration + settle) / dt below is exact
# the clean durations of the four paths in periods: 8 exactly; the others end inside a period
CLOCK_PERIODS = np.array([8.0, 3.3, 5.3, 9.5])


def clock_case():
    c = rollout_case("panda")
    nb = len(CLOCK_PERIODS)
    return dict(c, dur=CLOCK_PERIODS * CLOCK_DT, q=c["q"][:nb], qd=c["qd"][:nb], qdd=c["qdd"][:nb], settle=0.0,
                model=tuple(None if a is None else a[:nb] for a in c["model"]), plant=tuple(None if a is None else a[:nb] for a in c["plant"]))


def clock_restatement(c, dur, **kw):
    return fr.rollout_batch(c["desc"], c["eef"], dur, c["q"], c["qd"], c["qdd"], c["kp"], c["kd"], c["tau_max"], dt=CLOCK_DT, settle=0.0,
                            n_samples=MO, feedforward=2, model_payload=c["model"], plant_payload=c["plant"], **kw)


def test_the_clock_edges(capi):
    """Through gto_track_rollout_device, where the device alone sees the durations and the payload masses: a path with no
    period at all, one with GTO_TRACK_MAX_STEPS + 1 of them (it must fail at once: a workgroup walks to the largest step
    count of its GOOD paths), payload masses of -1 and NaN, and beside them a path of exactly 8 periods."""
    import torch
    c = clock_case()
    h = capi.SolverHandle(c["desc"], c["ee"], c["gr"], device=0, n_gripper_points=c["ngp"])
    stream = torch.cuda.Stream(device="cuda:0")
    assert (8 * CLOCK_DT) / CLOCK_DT == 8.0 and np.ceil((MAX_STEPS + 0.5) * CLOCK_DT / CLOCK_DT) == MAX_STEPS + 1

    def run(dur=None, model_mass=None, plant_mass=None):
        cc = dict(c, dur=c["dur"] if dur is None else dur)
        if model_mass is not None:
            cc["model"] = (model_mass,) + tuple(c["model"][1:])
        if plant_mass is not None:
            cc["plant"] = (plant_mass,) + tuple(c["plant"][1:])
        tensors = to_device(cc, cc["q"])
        out = device_rollout(h, cc, "full", tensors, stream, dt=CLOCK_DT, settle=0.0)
        stream.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    clean = run()
    want = clock_restatement(c, c["dur"])
    assert want["clip_margin"].min() > 1e-9 and want["steps"].tolist() == [8, 4, 6, 10]
    assert (clean["status"] == 0).all() and np.array_equal(clean["steps"], want["steps"]) and np.array_equal(clean["sat_steps"], want["sat_steps"])
    assert same(clean["t"], want["t"])
    err = {k: np.abs(clean[k] - want[k]).max() for k in ("q", "qd", "err_max", "err_end")}
    print(f"clock: steps {clean['steps'].tolist()} differences {err}, allowed {16 * ROLLOUT_D:.2e}")
    assert max(err.values()) <= 16 * ROLLOUT_D
    edge = c["dur"].copy()
    edge[1], edge[3] = 0.0, (MAX_STEPS + 0.5) * CLOCK_DT
    m, p = c["model"][0], c["plant"][0]
    cases = {"no period, too many": (dict(dur=edge), [1, 3]),
             "plant mass": (dict(plant_mass=np.array([p[0], -1.0, p[2], np.nan])), [1, 3]),
             "model mass": (dict(model_mass=np.array([np.nan, m[1], -1.0, m[3]])), [0, 2])}
    assert clock_restatement(c, edge)["status"].tolist() == [0, 2, 0, 2]
    for what, (kw, rows) in cases.items():
        got = run(**kw)
        bad = np.zeros(len(edge), dtype=bool)
        bad[rows] = True
        assert np.array_equal(got["status"], np.where(bad, 2, 0)), (what, got["status"])
        assert not got["steps"][bad].any() and not got["sat_steps"][bad].any(), what
        for k in got:
            if k in ("q", "qd", "t", "err_max", "err_end"):
                assert np.isnan(got[k][bad]).all(), (what, k)
            assert same(got[k][~bad], clean[k][~bad]), (what, k)
    h.close()


# ------------------------------------------------------------------------------------------------ the Python layers
TRACK_OUT = ("err_max", "err_end", "sat_steps", "status")


def test_chain_planner_and_utils_go_through_the_rollout(capi):
    """The fixture of tests/test_gpu_retime_torque.py's layer test: two objects with three grasps each, a lift of four steps."""
    import grasptrajopt_amd as g
    from grasptrajopt_amd import utils
    from grasptrajopt_amd.grasp_chain import GraspChain
    from test_gpu_grasp_chain import chain_setup
    nb, n, ns = 2, 3, 30
    cfg, robot, fields, RT = chain_setup("panda", nb * n, seed=21)
    dr.with_fixture_inertials(robot.desc, "panda")
    RT = RT.reshape(nb, n, 4, 4)
    qc = np.array(cfg["default_pose"], dtype=np.float64)
    chain = GraspChain(robot, cfg["link_ee"], cfg["link_gripper"])
    chain.max_iter = 20
    vm, am = robot.desc.velocity, np.full(robot.ndof, 0.5)
    held = dict(mass=[2.0, 0.5], com=[[0.0, 0.0, 0.05], [0.02, 0.0, 0.0]])
    rt = dict(vmax=vm, amax=am, n_samples=ns, profile="torque", payload=held)
    args, kw = (qc, RT, RT, [n, n], fields[0], np.array([0.01, -0.02, 0.0])), dict(axis_standoff=cfg["axis_standoff"])
    lift = dict(mode="lift", distance=0.1, steps=4)
    kp = np.array([600.0, 600, 600, 600, 250, 150, 50, 0, 0])
    kd = np.array([50.0, 50, 50, 20, 20, 20, 10, 0, 0])
    trk = dict(kp=kp, kd=kd, dt=4e-3, settle=0.02, feedforward="full")
    h = chain._handle
    plain = chain.plan_objects(*args, retrieve=lift, retime=dict(rt, retrieve_samples=True), **kw)
    none = chain.plan_objects(*args, retrieve=lift, retime=dict(rt, retrieve_samples=True), track=None, **kw)
    tracked = chain.plan_objects(*args, retrieve=lift, retime=dict(rt, retrieve_samples=True), track=trk, **kw)
    new = {p + k for p in ("track_", "retrieve_track_") for k in TRACK_OUT}
    assert set(vars(none)) == set(vars(plain)) and set(vars(tracked)) == set(vars(plain)) | new
    for k, v in vars(plain).items():  # the option changes nothing else, and without it the chain is what it was
        assert same(v, getattr(none, k)) and same(v, getattr(tracked, k)), k
    approach = h.retime_paths_torque(tracked.plans, vm, am, n_samples=ns)  # an empty hand
    want = h.track_rollout(approach["duration"], approach["q"], approach["qd"], approach["qdd"], **trk)
    for k in TRACK_OUT:
        assert same(getattr(tracked, "track_" + k), want[k]), k
    assert (want["status"] == 0).all() and (want["steps"] > 100).all()
    want = h.track_rollout(tracked.retrieve_durations, tracked.retrieve_q, tracked.retrieve_qd, tracked.retrieve_qdd,
                           model_payload=held, plant_payload=held, **trk)
    for k in TRACK_OUT:
        assert same(getattr(tracked, "retrieve_track_" + k), want[k]), k
    assert (want["status"] == 0).all()
    # the chain's own sample buffers, and a controller that does not know what it holds
    blind = chain.plan_objects(*args, retrieve=lift, retime=rt, track=dict(trk, model_payload=None), **kw)
    assert not hasattr(blind, "retrieve_q") and same(blind.track_err_max, tracked.track_err_max)
    want = h.track_rollout(tracked.retrieve_durations, tracked.retrieve_q, tracked.retrieve_qd, tracked.retrieve_qdd,
                           model_payload=None, plant_payload=held, **trk)
    for k in TRACK_OUT:
        assert same(getattr(blind, "retrieve_track_" + k), want[k]), k
    assert blind.retrieve_track_err_max[0] > tracked.retrieve_track_err_max[0]  # 2 kg nobody told the controller about
    with pytest.raises(ValueError, match="needs retime"):
        chain.plan_objects(*args, retrieve=lift, track=trk, **kw)
    with pytest.raises(TypeError, match="kp and kd"):
        chain.plan_objects(*args, retrieve=lift, retime=rt, track=dict(kp=kp), **kw)
    with pytest.raises(ValueError, match="kp"):
        chain.plan_objects(*args, retrieve=lift, retime=rt, track=dict(trk, kp=-1.0), **kw)
    # GTOPlanner.retrieve_path: the same rollout of the first object's retrieve path
    planner = g.GTOPlanner(robot, cfg["link_ee"], cfg["link_gripper"])
    one = dict(mass=2.0, com=[0.0, 0.0, 0.05])
    path, reached, traj = planner.retrieve_path(tracked.plans[0], "lift", distance=0.1, steps=4, retime=dict(rt, payload=one),
                                                track=dict(trk, n_samples=11))
    assert {"track_" + k for k in capi.TRACK_KEYS} <= set(traj) and traj["track_q"].shape == (11, robot.ndof)
    for k in TRACK_OUT:
        assert traj["track_" + k] == getattr(tracked, "retrieve_track_" + k)[0], k
    with pytest.raises(ValueError, match="needs retime"):
        planner.retrieve_path(tracked.plans[0], "lift", distance=0.1, steps=4, track=trk)
    with pytest.raises(TypeError, match="kp and kd"):
        planner.retrieve_path(tracked.plans[0], "lift", distance=0.1, steps=4, retime=dict(rt, payload=one), track=dict(trk, gain=1))
    # utils.track_trajectories on a retimed dict
    retimed = utils.retime_paths(robot, tracked.retrieve_path, alim=am, n_samples=ns, profile="torque", payload=held, link_ee=cfg["link_ee"])
    u = utils.track_trajectories(robot, retimed, kp, kd, dt=4e-3, settle=0.02, n_samples=9, model_payload=held, plant_payload=held,
                                 link_ee=cfg["link_ee"])
    want = h.track_rollout(retimed["duration"], retimed["q"], retimed["qd"], retimed["qdd"], kp, kd, dt=4e-3, settle=0.02, n_samples=9,
                           model_payload=held, plant_payload=held)
    assert set(u) == set(capi.TRACK_KEYS)
    for k in u:
        assert same(u[k], want[k]), k
    for k in TRACK_OUT:
        assert same(u[k], getattr(tracked, "retrieve_track_" + k)), k
    with pytest.raises(ValueError, match="needs link_ee"):
        utils.track_trajectories(robot, retimed, kp, kd, plant_payload=held)
    with pytest.raises(ValueError, match="lacks"):
        utils.track_trajectories(robot, dict(duration=retimed["duration"]), kp, kd)
    chain.close() if hasattr(chain, "close") else None
