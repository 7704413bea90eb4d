"""GPU: gto_retime_batch[_device] against the numpy restatement (tests/retime_ref.py), the limits and ends derived from
its own outputs, LPs, edge cases, bit-identical repeats, and the Python surface."""
import json
import os

import numpy as np
import pytest

from grasptrajopt_amd import _capi, synthetic as syn
from grasptrajopt_amd.robot_desc import load_builtin
import retime_ref as rr

pytestmark = pytest.mark.gpu

# Tolerances, once.  Against the restatement: |gpu - ref| <= tol * max(max|ref|, 1) per array (the spline slopes come from a
# Thomas solve here and from LAPACK's banded solver in scipy: both FP64, different round-off).  RTOL holds for x = sdot^2
# everywhere, and for sdot, the segment times, the duration and the samples of every plan whose profile does not come to
# rest inside the path.  SQRT_RTOL holds only where it does: at an interior gridpoint with x = 0 up to round-off (~1e-17,
# "a rest"), sdot = sqrt(x) turns that round-off into ~1e-8, in sdot there, in the times of the two segments next to it and
# so in the instants of the samples.  qddot jumps at gridpoints (constant acceleration per segment), so samples within
# 1e-9 duration of a gridpoint time are left out of its comparison: there round-off alone picks the segment.
RTOL = 1e-9
SQRT_RTOL = 1e-6
PATH_ATOL = 1e-12   # q on the spline, and at the ends equal to the waypoints
LIMIT_SLACK = 1e-9  # limits derived from the outputs: <= limit * (1 + LIMIT_SLACK)
LP_RTOL = 1e-6      # controllable sets and forward steps of independent LPs against the GPU's profile
REST = 1e-12        # an interior x <= REST * max x is a rest
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("duration", "t_grid", "sd_grid", "q", "qd", "qdd")


def _cfg(robot):
    return json.load(open(os.path.join(ROOT, "grasptrajopt_amd", "data", f"{robot}_cfg.json")))


def _handle(name, T):
    desc = load_builtin(name)
    cfg = _cfg(name.replace("_mobile", ""))
    o = _capi.default_opts()
    o.T = T
    return desc, cfg, _capi.SolverHandle(desc, cfg["link_ee"], cfg["link_gripper"], o, device=0)


@pytest.fixture(scope="module")
def panda():
    desc, cfg, h = _handle("panda", 50)
    yield desc, cfg, h
    h.close()


@pytest.fixture(scope="module")
def fetch():
    desc, cfg, h = _handle("fetch_mobile", 80)
    yield desc, cfg, h
    h.close()


def _solved_plans(desc, cfg, h, B):
    sc = syn.make_scene(3, n=48, res=0.0467)
    h.set_scene(0, sc.c_all, sc.c_obs, sc.shape, sc.origin, sc.res)
    RT, qg = syn.make_goals(desc, h.eval_fk, cfg["link_ee"], B, seed=5)
    qc = np.array(cfg["default_pose"])
    Q0 = np.stack([syn.make_seed(qc, qg[i], h.T, desc.param_index) for i in range(B)])
    S = syn.standoff_pose(-0.1, cfg["axis_standoff"])
    h.set_opts(max_iter=30)
    Q, _, _, _, _ = h.solve_batch(0, np.tile(qc, (B, 1)), RT.reshape(B, 1, 16), 1, S, [0, 0, 0], Q0)
    return Q, (qc, RT, S, Q0)


def _same(a, b):
    """Bit for bit, NaN for NaN (a plan whose profile rests at two neighbouring gridpoints exactly has an infinite
    duration, status GTO_STATUS_NUMERICAL and NaN samples)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _limits(desc):
    return desc.velocity, np.full(desc.ndof, 0.5)


def _close(a, b, rtol=RTOL):
    a, b = np.asarray(a), np.asarray(b)
    scale = max(np.abs(b).max(initial=0.0), 1.0)
    assert np.all(np.abs(a - b) <= rtol * scale), f"max |diff| {np.abs(a - b).max():.3e}, scale {scale:.3e}"


def _check_against_ref(desc, h, plans, subdiv=2, M=100, vmax=None, amax=None):
    vm, am = _limits(desc) if desc.velocity is not None else (None, None)
    vm = vm if vmax is None else vmax
    am = am if amax is None else amax
    g = h.retime_batch(plans, vm, am, subdiv=subdiv, n_samples=M)
    r = rr.retime(plans, vm, am, subdiv, M)
    assert np.array_equal(g["status"], r["status"])
    _close(g["sd_grid"] ** 2, r["sd_grid"] ** 2)
    for b in np.nonzero(r["status"] == 0)[0]:
        x = r["sd_grid"][b] ** 2
        rest = np.zeros(x.shape, bool)
        rest[1:-1] = x[1:-1] <= REST * x.max()
        near = rest[:-1] | rest[1:]                  # segments next to a rest
        _close(g["sd_grid"][b][~rest], r["sd_grid"][b][~rest])
        _close(g["sd_grid"][b][rest], r["sd_grid"][b][rest], SQRT_RTOL)
        dt_g, dt_r = np.diff(g["t_grid"][b]), np.diff(r["t_grid"][b])
        assert np.all(np.abs(dt_g - dt_r)[~near] <= RTOL * dt_r[~near])
        assert np.all(np.abs(dt_g - dt_r)[near] <= SQRT_RTOL * dt_r[near])
        allow = RTOL * r["duration"][b] + SQRT_RTOL * dt_r[near].sum()
        assert np.all(np.abs(g["t_grid"][b] - r["t_grid"][b]) <= allow)
        assert abs(g["duration"][b] - r["duration"][b]) <= allow
        tol = SQRT_RTOL if rest.any() else RTOL
        _close(g["q"][b], r["q"][b], tol)
        _close(g["qd"][b], r["qd"][b], tol)
        ts = np.linspace(0, r["duration"][b], M)
        far = np.abs(ts[:, None] - r["t_grid"][b][None, 1:-1]).min(axis=1) > 1e-9 * r["duration"][b] if r["duration"][b] > 0 else np.ones(M, bool)
        _close(g["qdd"][b][far], r["qdd"][b][far], tol)
    bad = r["status"] != 0
    assert np.all(np.isnan(g["q"][bad])) and np.all(np.isnan(g["qdd"][bad]))
    return g


def _converged(g, n=None):
    return np.nonzero(g["status"] == 0)[0][:n]


def _derived_checks(desc, plans, g, vmax, amax, subdiv=2):
    B, nd, T = plans.shape
    N = subdiv * (T - 1) + 1
    for b in range(B):
        moving = np.any(plans[b] != plans[b][:, :1], axis=1)
        sp, s, p1, p2 = rr.path_derivatives(plans[b], subdiv)
        p1[:, ~moving] = 0.0
        p2[:, ~moving] = 0.0
        sd = g["sd_grid"][b]
        x = sd ** 2
        u = (x[1:] - x[:-1]) * 0.5 * (N - 1)
        fin = np.isfinite(vmax)
        assert np.all(np.abs(p1[:, fin]) * sd[:, None] <= vmax[fin] * (1 + LIMIT_SLACK) + 1e-300)
        acc = np.abs(p1[:-1] * u[:, None] + p2[:-1] * x[:-1, None])
        assert np.all(acc <= amax * (1 + LIMIT_SLACK))
        # ends: at rest on the first and last waypoint
        np.testing.assert_allclose(g["q"][b][0], plans[b][:, 0], rtol=0, atol=PATH_ATOL)
        np.testing.assert_allclose(g["q"][b][-1], plans[b][:, -1], rtol=0, atol=PATH_ATOL)
        np.testing.assert_allclose(g["qd"][b][[0, -1]], 0.0, rtol=0, atol=1e-9 * max(1.0, np.abs(g["qd"][b]).max()))
        assert g["duration"][b] > 0 and sd[0] == 0 and sd[-1] == 0
        # path: every sample lies on scipy's spline at the position the GPU's own grid implies
        ts = np.linspace(0, g["duration"][b], g["q"].shape[1])
        t = g["t_grid"][b]
        i = np.clip(np.searchsorted(t, ts, side="right") - 1, 0, N - 2)
        tau = ts - t[i]
        ss = np.clip(s[i] + tau * (sd[i] + 0.5 * u[i] * tau), 0, 1)
        np.testing.assert_allclose(g["q"][b], sp(ss), rtol=0, atol=PATH_ATOL)


def test_random_plans_panda(panda):
    desc, cfg, h = panda
    plans = rr.random_plans(desc, 256, 50, seed=1)
    g = _check_against_ref(desc, h, plans)
    sel = _converged(g, 32)
    _derived_checks(desc, plans[sel], {k: v[sel] for k, v in g.items()}, *_limits(desc))
    assert g["t_grid"].shape == (256, 99) and g["q"].shape == (256, 100, 9)


def test_solved_plans_panda(panda):
    desc, cfg, h = panda
    Q, _ = _solved_plans(desc, cfg, h, 16)
    g = _check_against_ref(desc, h, Q)
    _derived_checks(desc, Q, g, *_limits(desc))


def test_fetch_mobile_T80(fetch):
    desc, cfg, h = fetch
    assert desc.n_opt == 10
    plans = rr.random_plans(desc, 64, 80, seed=2)
    g = _check_against_ref(desc, h, plans)
    assert np.all(g["status"] == 0)
    sel = _converged(g, 16)
    _derived_checks(desc, plans[sel], {k: v[sel] for k, v in g.items()}, *_limits(desc))
    assert g["t_grid"].shape == (64, 159)


def test_subdiv_and_samples(panda):
    desc, cfg, h = panda
    plans = rr.random_plans(desc, 8, 50, seed=9)
    _check_against_ref(desc, h, plans, subdiv=5, M=37)
    _check_against_ref(desc, h, plans, subdiv=1, M=2)


def test_lp_controllable_sets(panda):
    desc, cfg, h = panda
    plans = rr.random_plans(desc, 8, 50, seed=4)
    vm, am = _limits(desc)
    g = h.retime_batch(plans, vm, am)
    for b in range(8):
        moving = np.any(plans[b] != plans[b][:, :1], axis=1)
        _, _, p1, p2 = rr.path_derivatives(plans[b], 2)
        p1[:, ~moving] = 0.0
        p2[:, ~moving] = 0.0
        x = g["sd_grid"][b] ** 2
        # every x_i lies in the controllable set an independent LP finds, and every step goes to the largest x_{i+1}
        # that the next controllable set admits (an all-zero profile fails this)
        for i in (1, 30, 60, 96):
            xl = rr.controllable_lp(p1, p2, vm, am, i)
            assert x[i] <= xl * (1 + LP_RTOL)
            xs = rr.step_lp(p1, p2, vm, am, i - 1, x[i - 1], xl)
            assert x[i] == pytest.approx(xs, rel=LP_RTOL, abs=1e-12)
        assert x[1] > 0 and x[48] > 0


def test_plan_that_rests_before_the_end_is_numerical(panda):
    """Plan 121 of this batch: the greedy forward pass reaches the edge of the controllable set at gridpoint N-3, from
    which the only continuation is x = 0 at N-2; the last segment then runs between two zeros."""
    desc, cfg, h = panda
    plans = rr.random_plans(desc, 256, 50, seed=1)
    g = h.retime_batch(plans[118:124], *_limits(desc))
    assert g["status"].tolist() == [0, 0, 0, rr.GTO_STATUS_NUMERICAL, 0, 0]
    sd = g["sd_grid"][3]
    assert sd[-2] <= 1e-3 * sd.max() and np.all(np.isnan(g["q"][3]))
    assert np.all(g["duration"][[0, 1, 2, 4, 5]] < 10)
    assert rr.retime(plans[121:122], *_limits(desc))["status"][0] == rr.GTO_STATUS_NUMERICAL


def test_stationary_plan(panda):
    desc, cfg, h = panda
    plans = rr.random_plans(desc, 3, 50, seed=5)
    plans[1] = plans[1][:, :1]
    g = h.retime_batch(plans, *_limits(desc))
    assert g["status"][1] == 0 and g["duration"][1] == 0
    assert np.all(g["t_grid"][1] == 0) and np.all(g["sd_grid"][1] == 0)
    assert np.all(g["q"][1] == plans[1][:, 0]) and np.all(g["qd"][1] == 0) and np.all(g["qdd"][1] == 0)
    assert g["duration"][0] > 0 and g["duration"][2] > 0


def test_nan_plan_leaves_neighbours_bit_identical(panda):
    desc, cfg, h = panda
    plans = rr.random_plans(desc, 9, 50, seed=6)
    clean = h.retime_batch(plans, *_limits(desc))
    bad = plans.copy()
    bad[4, 2, 17] = np.nan
    g = h.retime_batch(bad, *_limits(desc))
    assert g["status"][4] == rr.GTO_STATUS_NUMERICAL and np.isnan(g["duration"][4])
    keep = np.arange(9) != 4
    for k in KEYS + ("status",):
        assert _same(g[k][keep], clean[k][keep]), k


def test_infinite_velocity_limits(panda):
    desc, cfg, h = panda
    plans = rr.random_plans(desc, 16, 50, seed=7)
    vm = desc.velocity.copy()
    vm[[0, 3, 5]] = np.inf
    g = _check_against_ref(desc, h, plans, vmax=vm)
    sel = _converged(g)
    _derived_checks(desc, plans[sel], {k: v[sel] for k, v in g.items()}, vm, np.full(desc.ndof, 0.5))


def test_invalid_arguments(panda):
    desc, cfg, h = panda
    plans = rr.random_plans(desc, 2, 50, seed=8)
    vm, am = _limits(desc)
    bad_a = am.copy()
    bad_a[2] = 0.0
    for kw in (dict(amax=bad_a), dict(amax=-am), dict(amax=np.full(desc.ndof, np.inf)), dict(vmax=np.zeros(desc.ndof)),
               dict(vmax=np.full(desc.ndof, np.nan)), dict(n_samples=1), dict(subdiv=0), dict(subdiv=30)):
        args = dict(vmax=vm, amax=am, subdiv=2, n_samples=100)
        args.update(kw)
        with pytest.raises(_capi.GTOError, match=r"\(-1\)"):
            h.retime_batch(plans, **args)


def test_empty_batch(panda):
    desc, cfg, h = panda
    g = h.retime_batch(np.empty((0, desc.ndof, 50)), *_limits(desc))
    assert g["duration"].shape == (0,) and g["q"].shape == (0, 100, desc.ndof)
    h.retime_batch_device(0, None, *_limits(desc), 2, 100)


def test_finger_limits_do_not_matter(panda):
    desc, cfg, h = panda
    Q, _ = _solved_plans(desc, cfg, h, 8)
    vm, am = _limits(desc)
    tiny = vm.copy()
    tiny[desc.param_index] = 1e-9
    a, b = h.retime_batch(Q, vm, am), h.retime_batch(Q, tiny, am)
    for k in KEYS + ("status",):
        assert _same(a[k], b[k]), k


def test_bit_identical_repeats_and_batches(panda):
    desc, cfg, h = panda
    plans = rr.random_plans(desc, 2048, 50, seed=10)
    lim = _limits(desc)
    a, b = h.retime_batch(plans, *lim), h.retime_batch(plans, *lim)
    for k in KEYS + ("status",):
        assert _same(a[k], b[k]), k
    for i in (0, 777, 2047):
        one = h.retime_batch(plans[i:i + 1], *lim)
        for k in KEYS:
            assert _same(one[k][0], a[k][i]), (k, i)


def _device_retime(h, Qd, B, desc, lim, M=100, N=99):
    import torch
    dev = Qd.device
    out = dict(duration=torch.empty(B, dtype=torch.float64, device=dev),
               t_grid=torch.empty((B, N), dtype=torch.float64, device=dev),
               sd_grid=torch.empty((B, N), dtype=torch.float64, device=dev),
               q=torch.empty((B, M, desc.ndof), dtype=torch.float64, device=dev),
               qd=torch.empty((B, M, desc.ndof), dtype=torch.float64, device=dev),
               qdd=torch.empty((B, M, desc.ndof), dtype=torch.float64, device=dev),
               status=torch.empty(B, dtype=torch.int32, device=dev))
    h.retime_batch_device(B, Qd.data_ptr(), *lim, 2, M, *(out[k].data_ptr() for k in KEYS + ("status",)))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_host_and_device_variants_agree(panda):
    import torch
    desc, cfg, h = panda
    plans = rr.random_plans(desc, 64, 50, seed=12)
    lim = _limits(desc)
    a = h.retime_batch(plans, *lim)
    b = _device_retime(h, torch.from_numpy(plans).to("cuda:0"), 64, desc, lim)
    for k in KEYS + ("status",):
        assert _same(a[k], b[k]), k


def test_device_variant_fed_by_the_solver(panda):
    import torch
    desc, cfg, h = panda
    B = 8
    Qh, (qc, RT, S, Q0) = _solved_plans(desc, cfg, h, B)
    cu = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to("cuda:0")
    sid, ng = cu(np.zeros(B), torch.int32), cu(np.ones(B), torch.int32)
    Qd = torch.empty((B, desc.ndof, 50), dtype=torch.float64, device="cuda:0")
    h.solve_batch_device(B, 1, sid.data_ptr(), cu(np.tile(qc, (B, 1))).data_ptr(), cu(RT.reshape(B, 1, 16)).data_ptr(),
                         ng.data_ptr(), cu(np.tile(S.reshape(1, 16), (B, 1))).data_ptr(), cu(np.zeros((B, 3))).data_ptr(),
                         cu(Q0).data_ptr(), Qd.data_ptr(), None, None, None, None)
    lim = _limits(desc)
    b = _device_retime(h, Qd, B, desc, lim)
    assert np.all(np.isfinite(Qd.cpu().numpy()))
    a = h.retime_batch(Qd.cpu().numpy(), *lim)
    for k in KEYS + ("status",):
        assert _same(a[k], b[k]), k


def test_python_surface(panda):
    import grasptrajopt_amd as g
    from grasptrajopt_amd.gto_models import GTORobotModel
    from grasptrajopt_amd import utils
    desc, cfg, h = panda
    robot = GTORobotModel(desc=load_builtin("panda"), param_joints=cfg["param_joints"], device=0)
    plans = rr.random_plans(desc, 4, 50, seed=13)
    r = utils.retime_plans(robot, plans)
    c = h.retime_batch(plans, desc.velocity, 0.5)
    for k in KEYS + ("status",):
        assert _same(r[k], c[k]), k
    qs, qds, qdds, ts = utils.convert_plan_to_trajectory_toppra(robot, plans[2])
    assert _same(qs, c["q"][2]) and _same(qds, c["qd"][2]) and _same(qdds, c["qdd"][2])
    assert _same(ts, np.linspace(0, c["duration"][2], 100))
    with pytest.raises(NotImplementedError):
        utils.convert_plan_to_trajectory_toppra(robot, plans[2], is_show=True)
    fetch_robot = GTORobotModel(desc=load_builtin("fetch_mobile"), device=0)
    fp = rr.random_plans(fetch_robot.desc, 2, 80, seed=14)
    assert utils.retime_plans(fetch_robot, fp)["t_grid"].shape == (2, 159)
    assert g is not None


# ------------------------------------------------------------------------------------------ width and length
def _limit_handle(T):
    from helpers import limit_robot
    desc, ee = limit_robot("chain", n_opt=16)
    o = _capi.default_opts()
    o.T, o.standoff_offset = T, -2
    return desc, _capi.SolverHandle(desc, ee, ee, o, device=0)


def _moving_plans(desc, B, T, mask, seed):
    """random_plans with exactly the joints of `mask` moving (the others constant, parameter joints included)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.maximum(desc.lower, -3.0), np.minimum(desc.upper, 3.0)
    s = np.linspace(0.0, 1.0, T)
    a = lo + (hi - lo) * rng.uniform(0.2, 0.8, (B, desc.ndof))
    b = lo + (hi - lo) * rng.uniform(0.2, 0.8, (B, desc.ndof))
    P = a[..., None] + (b - a)[..., None] * (3 * s ** 2 - 2 * s ** 3)
    P += 0.05 * np.sin(2 * np.pi * rng.uniform(0.5, 2.0, (B, desc.ndof, 1)) * s + rng.uniform(0, 6, (B, desc.ndof, 1)))
    still = np.setdiff1d(np.arange(desc.ndof), mask)
    P[:, still] = P[:, still, :1]
    return P


def _wide_limits(desc):
    rng = np.random.default_rng(3)
    vm = rng.uniform(0.5, 2.5, desc.ndof)
    vm[::7] = np.inf
    return vm, rng.uniform(0.3, 1.5, desc.ndof)


@pytest.mark.parametrize("T", [50, 96])
@pytest.mark.parametrize("mask", ["all", "0,13,30", "15", "all but 7", "0,1,2,3,4,5,6,7,8,9,10"])
def test_limit_robot_moving_masks(T, mask):
    """The 31-joint chain of tests/helpers.limit_robot: every joint moving (31 acceleration lines and the link to the next
    gridpoint: 32 lines, 1024 pairs, 16 sweeps of the pass kernel's pair loop), the moving joints packed by a ballot prefix
    count from masks that are not contiguous ({0, 13, 30}, one joint alone, all but one) and the contiguous run tests had."""
    desc, h = _limit_handle(T)
    assert desc.ndof == 31
    m = {"all": np.arange(31), "all but 7": np.setdiff1d(np.arange(31), [7])}.get(mask)
    m = np.array([int(v) for v in mask.split(",")]) if m is None else m
    plans = _moving_plans(desc, 6, T, m, seed=len(m) + T)
    moving = np.any(plans != plans[:, :, :1], axis=2)
    assert (moving == np.isin(np.arange(31), m)[None]).all()
    vm, am = _wide_limits(desc)
    g = _check_against_ref(desc, h, plans, vmax=vm, amax=am)
    ok = _converged(g)
    assert len(ok) >= 4, g["status"]
    _derived_checks(desc, plans[ok], {k: v[ok] for k, v in g.items()}, vm, am)
    h.close()


@pytest.mark.parametrize("T,subdiv", [(94, 11), (4, 341), (50, 2)])
def test_limit_robot_longest_grid(T, subdiv):
    """N = subdiv (T - 1) + 1 = 1024 gridpoints, the most the pass kernel keeps in LDS, on the 31-joint chain with every joint
    moving; one gridpoint more is refused."""
    desc, h = _limit_handle(T)
    N = subdiv * (T - 1) + 1
    assert N in (1024, 99)
    plans = _moving_plans(desc, 3, T, np.arange(31), seed=T)
    vm, am = _wide_limits(desc)
    g = _check_against_ref(desc, h, plans, subdiv=subdiv, M=257, vmax=vm, amax=am)
    assert g["sd_grid"].shape == (3, N)
    ok = _converged(g)
    assert len(ok) >= 2, g["status"]
    _derived_checks(desc, plans[ok], {k: v[ok] for k, v in g.items()}, vm, am, subdiv=subdiv)
    h.close()
    if N == 1024:
        for T2, sd2 in ((5, 256), (33, 32)):   # N = 1025
            desc, h = _limit_handle(T2)
            with pytest.raises(_capi.GTOError, match=r"\(-1\): gto_retime_batch: subdiv \(T-1\) \+ 1 must be <= 1024"):
                h.retime_batch(_moving_plans(desc, 1, T2, np.arange(31), seed=1), vm, am, subdiv=sd2)
            h.close()


def test_joint_moving_by_1e_300_takes_the_overflow_path():
    """A joint that moves by ~1e-300 under a large acceleration limit: amax / |p1| overflows at every gridpoint, the joint
    bounds x through |p2 x| <= amax alone (rt_line's overflow path on the GPU, retime_ref._has_line in the restatement),
    and the plan is retimed by the other joints as if it stood still."""
    desc, h = _limit_handle(50)
    plans = _moving_plans(desc, 4, 50, np.arange(31), seed=9)
    s = np.linspace(0.0, 1.0, 50)
    plans[:, 12] = 1e-300 * (3 * s ** 2 - 2 * s ** 3)[None] * np.array([1.0, -2.0, 0.5, 3.0])[:, None]
    vm, am = _wide_limits(desc)
    am[12] = 1e12
    for b in range(4):
        _, _, p1, p2 = rr.path_derivatives(plans[b], 2)
        assert np.any(p1[:, 12] != 0) and not rr._has_line(p1[:, 12], p2[:, 12], np.full(len(p1), am[12])).any()
    g = _check_against_ref(desc, h, plans, vmax=vm, amax=am)
    ok = _converged(g)
    assert len(ok) >= 3, g["status"]
    _derived_checks(desc, plans[ok], {k: v[ok] for k, v in g.items()}, vm, am)
    # the same plans with joint 12 standing still: the same profile up to round-off
    still = plans.copy()
    still[:, 12] = 0.0
    g0 = h.retime_batch(still, vm, am)
    np.testing.assert_array_equal(g0["status"], g["status"])
    _close(g["sd_grid"][ok] ** 2, g0["sd_grid"][ok] ** 2)
    h.close()


def test_lp_every_gridpoint(panda):
    """The controllable set and the forward step of independent LPs at every interior gridpoint of N = 99 (not four)."""
    desc, cfg, h = panda
    plans = rr.random_plans(desc, 3, 50, seed=12)
    vm, am = _limits(desc)
    g = h.retime_batch(plans, vm, am)
    N = plans.shape[2] * 2 - 1
    for b in _converged(g):
        moving = np.any(plans[b] != plans[b][:, :1], axis=1)
        _, _, p1, p2 = rr.path_derivatives(plans[b], 2)
        p1[:, ~moving] = 0.0
        p2[:, ~moving] = 0.0
        x = g["sd_grid"][b] ** 2
        for i in range(1, N - 1):
            xl = rr.controllable_lp(p1, p2, vm, am, i)
            assert x[i] <= xl * (1 + LP_RTOL) + 1e-15, i
            xs = rr.step_lp(p1, p2, vm, am, i - 1, x[i - 1], xl)
            assert x[i] == pytest.approx(xs, rel=LP_RTOL, abs=1e-12), i
