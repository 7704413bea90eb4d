"""GPU: gto_retime_paths_torque[_device] against the restatement (tests/retime_torque_ref.py), against the torque limits
recomputed from its own outputs with the yardstick of tests/dynamics_ref.py, against the convex call on the same inputs,
tau_out against gto_inverse_dynamics, on other robots, on the largest grid, under batching and padding, at the edges of the
contract, and through the Python layers.  Every call goes through the C ABI.

Durations: the GPU's profile and the restatement's are both feasible and both certified, so both lie in
[T*, (1 + gap_tol) T*]: |d_gpu - d_ref| <= gap_tol d_ref, with (1 + RTOL) for the round-off of the sums.
Torques from the outputs: |tau_ij| <= tau_max_j (1 + LIMIT_SLACK) + 1e-11 max(1, |tau|_inf), the second term being the
project's bar for gto_inverse_dynamics against the yardstick (the rows were built by the kernel's own inverse dynamics)."""
import functools

import numpy as np
import pytest

from grasptrajopt_amd import _capi
import dynamics_cases as dc
import dynamics_ref as dr
import retime_convex_ref as cr
import retime_paths_ref as pr
import retime_ref as rr
import retime_torque_ref as tr
from test_gpu_retime import KEYS, LIMIT_SLACK, RTOL, _moving_plans, _same
from test_gpu_retime_convex import _recomputed

pytestmark = pytest.mark.gpu
ALL = KEYS + ("tau", "status", "iters")
GAP_TOL = 1e-8
AMAX = 50.0
ID_RTOL = 1e-11
NUMERICAL, MAX_ITER, INFEASIBLE = cr.GTO_STATUS_NUMERICAL, cr.GTO_STATUS_MAX_ITER, tr.GTO_STATUS_INFEASIBLE
KINDS = ("none", "mass", "full")


@pytest.fixture(scope="module")
def handles():
    """name -> (desc, end-effector frame, handle) of the robots of tests/dynamics_cases.py used here."""
    made = {}
    for name in ("panda", "chain_1", "limit_chain", "prismatic_only"):
        desc, ee, gr, ngp = dc.robot(name)
        made[name] = (desc, desc.frame_index(ee), _capi.SolverHandle(desc, ee, gr, device=0, n_gripper_points=ngp))
    yield made
    for *_, h in made.values():
        h.close()


def _payload(kind, B=pr.B):
    return dc.payloads(B, seed=31)[kind]


def _as_dict(pl, rows=slice(None)):
    return None if pl is None else {k: v[rows] for k, v in zip(("mass", "com", "inertia"), pl) if v is not None}


def _panda_inputs(Tp, mixed=False, batch=pr.B):
    desc, paths, n_cols, vm, _ = pr.inputs("panda", Tp, mixed, batch=batch)
    return paths, n_cols, np.asarray(vm, float), np.full(desc.ndof, AMAX)


@functools.lru_cache(maxsize=None)
def _reference(Tp, mixed, subdiv, kind, scale=1.0):
    desc, ee, _, _ = dc.robot("panda")
    paths, n_cols, vm, am = _panda_inputs(Tp, mixed)
    with np.errstate(divide="ignore", invalid="ignore"):
        return tr.retime_paths_torque_ref(desc, desc.frame_index(ee), paths, n_cols, vm, am, scale * desc.effort, _payload(kind), subdiv,
                                          pr.M, GAP_TOL)


def _torques_hold(desc, fee, paths, cols, g, tm, payload, subdiv, ID=None):
    """tau at every gridpoint i <= N-2 from sd_grid alone, by the yardstick (ID: another inverse dynamics, rows at once)."""
    worst = 0.0
    for b, C in enumerate(cols):
        N = subdiv * (C - 1) + 1
        if g["status"][b] in (NUMERICAL, INFEASIBLE) or N < 3:
            continue
        q, p1, p2, moving = tr.path_points(paths[b][:, :C], subdiv)
        if not moving.any():
            continue
        x = g["sd_grid"][b][:N] ** 2
        u = (x[1:] - x[:-1]) * 0.5 * (N - 1)
        qd, qdd = p1[:-1] * g["sd_grid"][b][:N - 1, None], p1[:-1] * u[:, None] + p2[:-1] * x[:-1, None]
        one = tr.payload_of(payload, b)
        tau = tr.tau_at(desc, fee, q[:-1], qd, qdd, one) if ID is None else ID(q[:-1], qd, qdd, one)
        bar = tm * (1 + LIMIT_SLACK) + ID_RTOL * max(1.0, np.abs(tau).max())
        worst = max(worst, np.max(np.abs(tau) / tm))
        assert np.all(np.abs(tau) <= bar), (b, np.max(np.abs(tau) - bar))
    return worst


def _tau_is_inverse_dynamics(h, g, payload, M):
    """tau_out: the bits of gto_inverse_dynamics on the returned samples, the path's payload repeated per sample."""
    B, _, nd = g["q"].shape
    pl = None if payload is None else tuple(None if a is None else np.repeat(a, M, axis=0) for a in payload)
    want = h.inverse_dynamics(g["q"].reshape(-1, nd), g["qd"].reshape(-1, nd), g["qdd"].reshape(-1, nd), _as_dict(pl))
    assert _same(g["tau"], want.reshape(B, M, nd))
    bad = np.isnan(g["q"]).all(axis=(1, 2))
    assert np.all(np.isnan(g["tau"][bad]).any(axis=(1, 2))) and np.all(np.isfinite(g["tau"][~bad]))


def _against_reference(desc, fee, h, paths, n_cols, vm, am, tm, payload, subdiv, r, M=pr.M):
    B, _, Tp = paths.shape
    cols = [Tp] * B if n_cols is None else [int(c) for c in n_cols]
    kw = dict(n_cols=n_cols, subdiv=subdiv, n_samples=M, gap_tol=GAP_TOL)
    convex = h.retime_paths_convex(paths, vm, am, **kw)
    g = h.retime_paths_torque(paths, vm, am, tau_max=tm, payload=_as_dict(payload), **kw)
    assert g["t_grid"].shape == (B, subdiv * (Tp - 1) + 1) and g["tau"].shape == (B, M, desc.ndof) and g["iters"].dtype == np.int32
    print("status", g["status"], r["status"], "iters", g["iters"], r["iters"])
    assert np.array_equal(g["status"], r["status"])
    for b, C in enumerate(cols):
        N = subdiv * (C - 1) + 1
        gt, gs = g["t_grid"][b], g["sd_grid"][b]
        if g["status"][b] == INFEASIBLE:
            assert g["iters"][b] == 0 and all(np.all(np.isnan(g[k][b])) for k in KEYS + ("tau",))
            continue
        assert _same(gt[N:], np.full(len(gt) - N, g["duration"][b])) and _same(gs[N:], np.zeros(len(gs) - N))
        if C == 1 or not np.any(paths[b][:, :C] != paths[b][:, :1]):
            assert g["status"][b] == 0 and g["duration"][b] == 0 and g["iters"][b] == 0 and np.all(gt == 0)
            assert np.all(g["q"][b] == paths[b][:, 0]) and np.all(g["qd"][b] == 0) and np.all(g["qdd"][b] == 0)
            continue
        if pr.unavoidable_stall(C, subdiv):
            assert g["status"][b] == NUMERICAL and np.isinf(g["duration"][b]) and np.all(np.isnan(g["q"][b])) and g["iters"][b] == 0
            continue
        assert g["status"][b] == 0 and 0 < g["iters"][b] <= _capi.RETIME_MAX_NEWTON // 2
        d_gpu, d_ref = g["duration"][b], r["duration"][b]
        print(f"b {b} C {C} subdiv {subdiv}: d_gpu {d_gpu!r} d_ref {d_ref!r} iters {g['iters'][b]} / {r['iters'][b]} convex {convex['duration'][b]!r}")
        assert abs(d_gpu - d_ref) <= GAP_TOL * d_ref * (1 + RTOL)
        assert d_gpu >= convex["duration"][b] * (1 - GAP_TOL)  # more rows: never shorter
    shown = dict(g, status=np.where(g["status"] == INFEASIBLE, NUMERICAL, g["status"]))
    _recomputed(paths, cols, shown, vm, am, subdiv, M)
    print("largest |tau| / tau_max at the gridpoints", _torques_hold(desc, fee, paths, cols, g, tm, payload, subdiv))
    _tau_is_inverse_dynamics(h, g, payload, M)
    return g, convex


# ------------------------------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("subdiv", pr.SUBDIVS)
@pytest.mark.parametrize("Tp", [2, 3, 5, 11])
def test_every_column_used(handles, Tp, subdiv, kind):
    desc, fee, h = handles["panda"]
    paths, _, vm, am = _panda_inputs(Tp)
    g, convex = _against_reference(desc, fee, h, paths, None, vm, am, desc.effort, _payload(kind), subdiv, _reference(Tp, False, subdiv, kind))
    if Tp >= 5 and subdiv == 2:  # the rows are active here (tests/test_retime_torque_cpu.py): the profile is strictly longer
        assert np.all(g["status"] == 0) and np.all(g["duration"] > convex["duration"] * (1 + 10 * GAP_TOL))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("subdiv", pr.SUBDIVS)
def test_mixed_counts(handles, subdiv, kind):
    desc, fee, h = handles["panda"]
    paths, n_cols, vm, am = _panda_inputs(pr.MIXED_TP, mixed=True)
    g, _ = _against_reference(desc, fee, h, paths, n_cols, vm, am, desc.effort, _payload(kind), subdiv,
                              _reference(pr.MIXED_TP, True, subdiv, kind))
    assert g["status"].tolist() == [0, NUMERICAL if subdiv == 1 else 0, 0, 0, 0]


def test_no_torque_limit_is_the_convex_profile(handles):
    desc, fee, h = handles["panda"]
    paths, n_cols, vm, am = _panda_inputs(pr.MIXED_TP, mixed=True)
    convex = h.retime_paths_convex(paths, vm, am, n_cols=n_cols, n_samples=pr.M, gap_tol=GAP_TOL)
    g = h.retime_paths_torque(paths, vm, am, tau_max=np.inf, payload=_as_dict(_payload("full")), n_cols=n_cols, n_samples=pr.M, gap_tol=GAP_TOL)
    assert np.array_equal(g["status"], convex["status"])
    assert np.all(np.abs(g["duration"] - convex["duration"]) <= GAP_TOL * convex["duration"] * (1 + RTOL))
    for k in KEYS + ("status", "iters"):  # no row is added: the same arithmetic
        assert _same(g[k], convex[k]), k


# ------------------------------------------------------------------------------------------ 2. other robots
def _other(name, Tp, subdiv, B, seed):
    """(paths, vmax, amax, tau_max): seeded paths with every joint moving; efforts 1.5 to 3 times the largest static torque
    along the paths (a joint that carries none: no limit)."""
    desc, ee, _, _ = dc.robot(name)
    fee = desc.frame_index(ee)
    paths = _moving_plans(desc, B, Tp, np.arange(desc.ndof), seed)
    rng = np.random.default_rng(seed)
    z = np.zeros(desc.ndof)
    top = np.zeros(desc.ndof)
    for b in range(B):
        q = tr.path_points(paths[b], subdiv)[0]
        top = np.maximum(top, np.abs(np.array([dr.inverse_dynamics(desc, qi, z, z, fee) for qi in q])).max(axis=0))
    tm = np.where(top > 1e-9, rng.uniform(1.5, 3.0, desc.ndof) * top, np.inf)
    return paths, rng.uniform(0.8, 2.0, desc.ndof), np.full(desc.ndof, AMAX), tm


@pytest.mark.parametrize("name,Tp,subdiv,B", [("chain_1", 4, 2, 5), ("chain_1", 5, 1, 5), ("limit_chain", 11, 2, 3), ("prismatic_only", 5, 2, 5)])
def test_other_robots(handles, name, Tp, subdiv, B):
    """chain_1: 2 frames, 64 rows per workgroup.  limit_chain: 32 frames, 17 rows per workgroup, 3 x 21 = 63 rows in four
    workgroups, the last ragged.  prismatic_only: g does not depend on q."""
    desc, fee, h = handles[name]
    paths, vm, am, tm = _other(name, Tp, subdiv, B, seed=Tp)
    pl = dc.payloads(B, seed=32)["full"]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = tr.retime_paths_torque_ref(desc, fee, paths, None, vm, am, tm, pl, subdiv, pr.M, GAP_TOL)
    g, _ = _against_reference(desc, fee, h, paths, None, vm, am, tm, pl, subdiv, r)
    assert np.any(g["status"] == 0)


# ------------------------------------------------------------------------------------------ 3. the largest grid
def test_the_largest_grid(handles):
    """N = 1024 gridpoints, one Panda path; the torques by gto_inverse_dynamics (the yardstick is too slow here)."""
    desc, fee, h = handles["panda"]
    paths = rr.random_plans(desc, 1, 1024, seed=4)
    vm, am = np.asarray(desc.velocity, float), np.full(desc.ndof, AMAX)
    pl = (np.array([1.0]), None, None)
    g = h.retime_paths_torque(paths, vm, am, payload=_as_dict(pl), subdiv=1, n_samples=pr.M)
    convex = h.retime_paths_convex(paths, vm, am, subdiv=1, n_samples=pr.M)
    print("iters", g["iters"], convex["iters"], "durations", g["duration"], convex["duration"])
    assert g["sd_grid"].shape == (1, 1024) and g["status"][0] == 0 and 0 < g["iters"][0] <= _capi.RETIME_MAX_NEWTON // 2
    assert g["duration"][0] >= convex["duration"][0] * (1 - GAP_TOL)
    ID = lambda q, qd, qdd, one: h.inverse_dynamics(q, qd, qdd, dict(mass=one[0]))
    worst = _torques_hold(desc, fee, paths, [1024], g, desc.effort, pl, 1, ID)
    print("largest |tau| / tau_max", worst)
    _recomputed(paths, [1024], g, vm, am, 1, pr.M)


# ------------------------------------------------------------------------------------------ 4. batch, position, padding
def _device_call(h, desc, paths, n_cols, lim, tm, payload, subdiv=2, M=pr.M, gap_tol=GAP_TOL, max_newton=_capi.RETIME_MAX_NEWTON):
    """gto_retime_paths_torque_device on a side stream, every output prefilled."""
    import torch
    B, _, Tp = paths.shape
    N = subdiv * (Tp - 1) + 1
    dev = "cuda:0"
    f64 = dict(dtype=torch.float64, device=dev)
    smp = lambda: torch.full((B, M, desc.ndof), -7.0, **f64)
    out = dict(duration=torch.full((B,), -7.0, **f64), t_grid=torch.full((B, N), -7.0, **f64), sd_grid=torch.full((B, N), -7.0, **f64),
               q=smp(), qd=smp(), qdd=smp(), tau=smp(), status=torch.full((B,), -7, dtype=torch.int32, device=dev),
               iters=torch.full((B,), -7, dtype=torch.int32, device=dev))
    up = lambda a, t=np.float64: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(dev)
    Pd, nc = up(paths), up(n_cols, np.int32)
    pl = [up(a) for a in (payload if payload is not None else (None, None, None))]
    ptr = lambda t: None if t is None else t.data_ptr()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    h.retime_paths_torque_device(B, Tp, Pd.data_ptr(), *lim, tau_max=tm, payload_mass=ptr(pl[0]), payload_com=ptr(pl[1]),
                                 payload_inertia=ptr(pl[2]), n_cols=ptr(nc), subdiv=subdiv, n_samples=M, gap_tol=gap_tol,
                                 max_newton=max_newton, **{k + "_out": out[k].data_ptr() for k in ALL}, stream=st.cuda_stream)
    st.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_batch_position_and_padding_do_not_change_a_bit(handles):
    desc, fee, h = handles["panda"]
    paths, _, vm, am = _panda_inputs(11, batch=9)
    cols = np.array([11, 3, 7, 2, 5, 9, 1, 4, 11], dtype=np.int32)
    pl = dc.payloads(9, seed=33)["full"]
    rev = tuple(a[::-1] for a in pl)
    tm = desc.effort
    for subdiv in pr.SUBDIVS:
        whole = _device_call(h, desc, paths, cols, (vm, am), tm, pl, subdiv)
        host = h.retime_paths_torque(paths, vm, am, tau_max=tm, payload=_as_dict(pl), n_cols=cols, subdiv=subdiv, n_samples=pr.M)
        back = _device_call(h, desc, paths[::-1], cols[::-1], (vm, am), tm, rev, subdiv)
        wide = np.full((9, desc.ndof, 19), np.nan)
        wide[:, :, :11] = paths
        padded = _device_call(h, desc, wide, cols, (vm, am), tm, pl, subdiv)
        assert (whole["status"] == 0).sum() >= (8 if subdiv == 2 else 7)
        for k in ALL:
            assert _same(whole[k], host[k]) and _same(whole[k], back[k][::-1]), k
        N11 = subdiv * 10 + 1
        for k in ("duration", "q", "qd", "qdd", "tau", "status", "iters"):
            assert _same(whole[k], padded[k]), k
        assert _same(padded["t_grid"][:, :N11], whole["t_grid"]) and _same(padded["sd_grid"][:, :N11], whole["sd_grid"])
        assert _same(padded["t_grid"][:, N11:], np.repeat(whole["duration"][:, None], padded["t_grid"].shape[1] - N11, axis=1))
        assert _same(padded["sd_grid"][:, N11:], np.zeros((9, padded["sd_grid"].shape[1] - N11)))
        for b in (0, 3, 6, 8):  # alone: the first path, two columns, one column, the last path
            one = _device_call(h, desc, paths[b:b + 1], cols[b:b + 1], (vm, am), tm, tuple(a[b:b + 1] for a in pl), subdiv)
            for k in ALL:
                assert _same(one[k][0], whole[k][b]), (k, b)
        # the payload travels with its path: another path's payload gives another profile where both are felt
        swapped = _device_call(h, desc, paths, cols, (vm, am), tm, tuple(np.roll(a, 1, axis=0) for a in pl), subdiv)
        assert not _same(swapped["duration"], whole["duration"])


# ------------------------------------------------------------------------------------------ 5. edges
def _heavy(pos, B=pr.B):
    """A payload no wrist of the Panda holds (40 kg, 0.3 m out) at the positions `pos`, none elsewhere."""
    mass, com = np.zeros(B), np.zeros((B, 3))
    mass[list(pos)], com[list(pos)] = 40.0, [0.3, 0.0, 0.0]
    return mass, com, None


def test_infeasible_paths_leave_their_neighbours(handles):
    desc, fee, h = handles["panda"]
    paths, n_cols, vm, am = _panda_inputs(pr.MIXED_TP, mixed=True)  # position 0 has one column: it must hold there too
    clean = _device_call(h, desc, paths, n_cols, (vm, am), desc.effort, _heavy(()))
    none = _device_call(h, desc, paths, n_cols, (vm, am), desc.effort, None)
    for k in ALL:
        assert _same(clean[k], none[k]), k
    assert np.all(clean["status"] == 0)
    for pos in ((0,), (2,), (4,), (0, 2, 4)):
        g = _device_call(h, desc, paths, n_cols, (vm, am), desc.effort, _heavy(pos))
        keep = np.setdiff1d(np.arange(pr.B), pos)
        assert np.all(g["status"][list(pos)] == INFEASIBLE) and np.all(g["iters"][list(pos)] == 0)
        for k in KEYS + ("tau",):
            assert np.all(np.isnan(g[k][list(pos)])), k
        for k in ALL:
            assert _same(g[k][keep], clean[k][keep]), (k, pos)


def test_a_path_that_rests_must_still_hold(handles):
    desc, fee, h = handles["panda"]
    paths, _, vm, am = _panda_inputs(5)
    still = np.repeat(paths[:, :, :1], 5, axis=2)
    z = np.zeros((pr.B, desc.ndof))
    grav = np.abs(h.inverse_dynamics(still[:, :, 0], z, z))
    g = h.retime_paths_torque(still, vm, am, n_samples=pr.M)
    assert np.all(g["status"] == 0) and np.all(g["duration"] == 0) and np.all(g["iters"] == 0)
    assert np.all(np.abs(g["tau"]) == grav[:, None, :])
    tm = 0.999 * grav.max(axis=0)
    cannot = (grav >= tm).any(axis=1)  # the rule itself, on the kernel's own static torques (none within 1e-3 of its limit)
    assert cannot.any()
    g = h.retime_paths_torque(still, vm, am, tau_max=tm, n_cols=[5, 1, 5, 1, 5], n_samples=pr.M)
    assert np.array_equal(g["status"], np.where(cannot, INFEASIBLE, 0))
    assert np.all(np.isnan(g["duration"][cannot])) and np.all(np.isnan(g["tau"][cannot])) and np.all(g["duration"][~cannot] == 0)
    g = h.retime_paths_torque(still, vm, am, tau_max=1.001 * grav.max(axis=0), n_cols=[5, 1, 5, 1, 5], n_samples=pr.M)
    assert np.all(g["status"] == 0)


@pytest.mark.parametrize("count", [0, -1, 12, 2 ** 31 - 1, -2 ** 31])
def test_a_wild_count_on_the_device_is_numerical_and_leaves_the_neighbours(handles, count):
    desc, fee, h = handles["panda"]
    paths, n_cols, vm, am = _panda_inputs(pr.MIXED_TP, mixed=True)
    pl = _payload("full")
    clean = _device_call(h, desc, paths, n_cols, (vm, am), desc.effort, pl)
    for pos in (0, 2, 4):
        c = n_cols.copy()
        c[pos] = count
        g = _device_call(h, desc, paths, c, (vm, am), desc.effort, pl)
        assert g["status"][pos] == NUMERICAL and g["iters"][pos] == 0
        for k in KEYS + ("tau",):
            assert np.all(np.isnan(g[k][pos])), k
        keep = np.arange(pr.B) != pos
        for k in ALL:
            assert _same(g[k][keep], clean[k][keep]), (k, pos)
        if count in (0, -1, 12):
            with pytest.raises(_capi.GTOError, match=r"\(-1\): gto_retime_paths_torque: n_cols must lie in \[1, Tp\]"):
                h.retime_paths_torque(paths, vm, am, n_cols=c)


def test_a_non_finite_payload_on_the_device_is_numerical_for_its_path_only(handles):
    desc, fee, h = handles["panda"]
    paths, n_cols, vm, am = _panda_inputs(pr.MIXED_TP, mixed=True)
    pl = _payload("full")
    clean = _device_call(h, desc, paths, n_cols, (vm, am), desc.effort, pl)
    for pos, what in ((0, "mass"), (3, "mass"), (4, "com"), (1, "inertia"), (3, "negative")):
        bad = tuple(a.copy() for a in pl)
        if what == "negative":
            bad[0][pos] = -1.0
        else:
            bad[("mass", "com", "inertia").index(what)][pos] = np.nan
        g = _device_call(h, desc, paths, n_cols, (vm, am), desc.effort, bad)
        assert g["status"][pos] == NUMERICAL and g["iters"][pos] == 0, (pos, what)
        for k in KEYS + ("tau",):
            assert np.all(np.isnan(g[k][pos])), k
        keep = np.arange(pr.B) != pos
        for k in ALL:
            assert _same(g[k][keep], clean[k][keep]), (k, pos, what)
    for what, arr in (("mass", [1.0, np.nan, 1, 1, 1]), ("mass", [1.0, -0.5, 1, 1, 1]), ("mass", [np.inf, 1, 1, 1, 1])):
        with pytest.raises(ValueError, match="payload: mass must be finite and >= 0"):
            h.retime_paths_torque(paths, vm, am, payload={what: arr}, n_cols=n_cols)


def test_the_newton_cap_leaves_a_feasible_profile(handles):
    desc, fee, h = handles["panda"]
    paths, n_cols, vm, am = _panda_inputs(pr.MIXED_TP, mixed=True)
    pl = _payload("mass")
    kw = dict(payload=_as_dict(pl), n_cols=n_cols, n_samples=pr.M)
    full = h.retime_paths_torque(paths, vm, am, **kw)
    g = h.retime_paths_torque(paths, vm, am, max_newton=1, **kw)
    assert g["status"].tolist() == [0, MAX_ITER, MAX_ITER, MAX_ITER, MAX_ITER] and g["iters"].tolist() == [0, 1, 1, 1, 1]
    assert all(np.all(np.isfinite(g[k])) for k in ("q", "qd", "qdd", "tau"))
    assert np.all(g["duration"][1:] > full["duration"][1:])
    _recomputed(paths, n_cols, g, vm, am, 2, pr.M)
    _torques_hold(desc, fee, paths, [int(c) for c in n_cols], g, desc.effort, pl, 2)
    capped = h.retime_paths_torque(paths, vm, am, max_newton=int(full["iters"].max()), **kw)
    for k in ALL:
        assert _same(capped[k], full[k]), k


def test_refusals_leave_the_handle_and_the_outputs(handles):
    import ctypes as C
    import torch
    from grasptrajopt_amd.robot_desc import load_builtin
    desc, fee, h = handles["panda"]
    paths, _, vm, am = _panda_inputs(5)
    before = h.retime_paths_torque(paths, vm, am, n_samples=pr.M)
    z = lambda Tp, B=1: np.zeros((B, desc.ndof, Tp))
    name = r"\(-1\): gto_retime_paths_torque: "
    for tm in (0.0, -3.0, np.nan, [87, 87, 87, 87, 12, 12, 0.0, 20, 20]):
        with pytest.raises(ValueError, match="tau_max must be > 0"):
            h.retime_paths_torque(paths, vm, am, tau_max=tm)
    # the library's own checks, through the raw entry points (the wrapper above refuses the same values first)
    pd = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    out = np.full(pr.B, -7.0)
    raw = lambda tm, pm=None, pc=None, pi=None, Tp=5, gap=1e-8, newton=10, subdiv=2: h.lib.gto_retime_paths_torque(
        h._h, pr.B, Tp, pd(paths), None, pd(vm), pd(am), None if tm is None else pd(tm), pm, pc, pi, subdiv, pr.M, gap, newton, pd(out),
        *([None] * 8))
    bad_tm = desc.effort.copy()
    bad_tm[3] = np.nan
    cases = [(dict(tm=bad_tm), "tau_max must be > 0"), (dict(tm=-desc.effort), "tau_max must be > 0"), (dict(tm=None), "null limit array"),
             (dict(tm=desc.effort, pc=pd(np.zeros((pr.B, 3)))), "payload_com / payload_inertia without payload_mass"),
             (dict(tm=desc.effort, pi=pd(np.zeros((pr.B, 6)))), "payload_com / payload_inertia without payload_mass"),
             (dict(tm=desc.effort, pm=pd([1, 1, -1, 1, 1])), "payload mass must be >= 0 and finite"),
             (dict(tm=desc.effort, pm=pd([1, 1, np.nan, 1, 1])), "payload mass must be >= 0 and finite"),
             (dict(tm=desc.effort, Tp=1), "Tp must be >= 2"), (dict(tm=desc.effort, gap=0.0), "gap_tol must be finite and > 0"),
             (dict(tm=desc.effort, newton=0), "max_newton must be >= 1"), (dict(tm=desc.effort, subdiv=0), "subdiv must be >= 1")]
    for kw, msg in cases:
        rc, said = raw(**kw), h.lib.gto_last_error(h._h).decode()
        assert rc == -1 and msg in said and "gto_retime_paths_torque: " in said, (kw, said)
        assert np.all(out == -7.0)
    for Tp, subdiv in ((1025, 1), (513, 2)):
        with pytest.raises(_capi.GTOError, match=name + r"subdiv \(Tp-1\) \+ 1 must be <= 1024"):
            h.retime_paths_torque(z(Tp), vm, am, subdiv=subdiv)
    with pytest.raises(_capi.GTOError, match=name + "null paths"):
        h.retime_paths_torque_device(1, 11, None, vm, am)
    h.retime_paths_torque_device(0, 11, None, vm, am)
    g = h.retime_paths_torque(np.empty((0, desc.ndof, 11)), vm, am, n_samples=pr.M)
    assert g["tau"].shape == (0, pr.M, desc.ndof) and g["iters"].shape == (0,)
    # a handle without inertials
    bare = load_builtin("panda")
    cfg = dc.robot("panda")
    hb = _capi.SolverHandle(bare, cfg[1], cfg[2], device=0)
    with pytest.raises(_capi.GTOError, match=r"\(-1\): no link inertials set"):
        hb.retime_paths_torque(paths, vm, am, tau_max=50.0)
    with pytest.raises(_capi.GTOError, match=r"\(-1\): no link inertials set"):
        hb.retime_paths_torque_device(0, 5, None, vm, am, tau_max=50.0)
    hb.close()
    # tau_out alone, every other output NULL
    Pd = torch.from_numpy(paths).to("cuda:0")
    tau = torch.empty((pr.B, pr.M, desc.ndof), dtype=torch.float64, device="cuda:0")
    h.retime_paths_torque_device(pr.B, 5, Pd.data_ptr(), vm, am, n_samples=pr.M, tau_out=tau.data_ptr(),
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _same(tau.cpu().numpy(), before["tau"])
    after = h.retime_paths_torque(paths, vm, am, n_samples=pr.M)
    for k in ALL:
        assert _same(before[k], after[k]), k


def test_the_greedy_and_convex_calls_are_what_they_were(handles):
    desc, fee, h = handles["panda"]
    paths, n_cols, vm, _ = _panda_inputs(pr.MIXED_TP, mixed=True)
    am = np.full(desc.ndof, 0.5)
    kw = dict(n_cols=n_cols, n_samples=pr.M)
    before = h.retime_paths(paths, vm, am, **kw), h.retime_paths_convex(paths, vm, am, **kw)
    h.retime_paths_torque(paths, vm, am, payload=_as_dict(_payload("full")), **kw)
    after = h.retime_paths(paths, vm, am, **kw), h.retime_paths_convex(paths, vm, am, **kw)
    for a, b in zip(before, after):
        for k in a:
            assert _same(a[k], b[k]), k


# ------------------------------------------------------------------------------------------ 6. the Python layers
def test_chain_planner_and_utils_go_through_the_torque_entry():
    import grasptrajopt_amd as g
    from grasptrajopt_amd import utils
    from grasptrajopt_amd.grasp_chain import GraspChain
    from test_gpu_grasp_chain import chain_setup
    B, n = 2, 3
    cfg, robot, fields, RT = chain_setup("panda", B * n, seed=21)
    dr.with_fixture_inertials(robot.desc, "panda")
    RT = RT.reshape(B, n, 4, 4)
    qc = np.array(cfg["default_pose"], dtype=np.float64)
    base = np.array([0.01, -0.02, 0.0])
    chain = GraspChain(robot, cfg["link_ee"], cfg["link_gripper"])
    chain.max_iter = 20
    vm, am = robot.desc.velocity, np.full(robot.ndof, AMAX)
    rt = dict(vmax=vm, amax=am, n_samples=pr.M)
    args, kw = (qc, RT, RT, [n, n], fields[0], base), dict(axis_standoff=cfg["axis_standoff"])
    h = chain._handle
    lift = dict(mode="lift", distance=0.1, steps=4)
    held = dict(mass=[2.0, 0.5], com=[[0.0, 0.0, 0.05], [0.02, 0.0, 0.0]])
    convex = chain.plan_objects(*args, retrieve=lift, retime=dict(rt, profile="convex", retrieve_samples=True), **kw)
    torque = chain.plan_objects(*args, retrieve=lift, retime=dict(rt, profile="torque", payload=held, retrieve_samples=True), **kw)
    # without the profile: the results of before
    again = chain.plan_objects(*args, retrieve=lift, retime=dict(rt, profile="convex", retrieve_samples=True), **kw)
    for k, v in vars(convex).items():
        assert _same(v, getattr(again, k)), k
    assert set(vars(torque)) == set(vars(convex)) | {"retrieve_tau"}
    for k, v in vars(convex).items():
        if "duration" not in k and "retime" not in k and k not in ("retrieve_q", "retrieve_qd", "retrieve_qdd"):
            assert _same(v, getattr(torque, k)), k
    want = h.retime_paths_torque(torque.plans, vm, am, n_samples=pr.M)  # the approach: an empty hand, the description's efforts
    assert _same(torque.durations, want["duration"]) and _same(torque.retime_status, want["status"])
    assert _same(torque.retime_iters, want["iters"])
    want = h.retime_paths_torque(torque.retrieve_path, vm, am, payload=held, n_samples=pr.M)
    assert _same(torque.retrieve_durations, want["duration"]) and _same(torque.retrieve_retime_status, want["status"])
    assert _same(torque.retrieve_retime_iters, want["iters"])
    for k in ("q", "qd", "qdd", "tau"):
        assert _same(getattr(torque, "retrieve_" + k), want[k]), k
    ok = (torque.retime_status == 0) & (convex.retime_status == 0)
    assert np.all(torque.durations[ok] >= convex.durations[ok] * (1 - GAP_TOL))
    for bad in (dict(tau_max=0.0), dict(tau_max=np.ones(3)), dict(payload=dict(mass=-1.0)), dict(payload=dict(com=[0, 0, 0])),
                dict(payload=dict(mass=[1.0, 2.0, 3.0]))):
        with pytest.raises(ValueError, match="tau_max|payload"):
            chain.plan_objects(*args, retrieve=lift, retime=dict(rt, profile="torque", **bad), **kw)
    # GTOPlanner.retrieve_path and utils
    planner = g.GTOPlanner(robot, cfg["link_ee"], cfg["link_gripper"])
    one = dict(mass=2.0, com=[0.0, 0.0, 0.05])
    path, reached, traj = planner.retrieve_path(torque.plans[0], "lift", distance=0.1, steps=4, retime=dict(rt, profile="torque", payload=one))
    assert _same(path, torque.retrieve_path[0]) and traj["duration"] == torque.retrieve_durations[0]
    assert traj["iters"] == torque.retrieve_retime_iters[0] and _same(traj["tau"], torque.retrieve_tau[0])
    path, reached, old = planner.retrieve_path(torque.plans[0], "lift", distance=0.1, steps=4, retime=dict(rt, profile="convex"))
    assert "tau" not in old and old["duration"] == convex.retrieve_durations[0]
    with pytest.raises(ValueError, match="tau_max"):
        planner.retrieve_path(torque.plans[0], "lift", distance=0.1, steps=4, retime=dict(rt, profile="torque", tau_max=-1.0))
    hu = robot.solver_handle(cfg["link_ee"], robot.desc.link_names[-1], role="util")
    want = h.retime_paths_torque(torque.retrieve_path, vm, am, tau_max=60.0, payload=held, n_cols=[3, 5], n_samples=pr.M, gap_tol=1e-6)
    u = utils.retime_paths(robot, torque.retrieve_path, n_cols=[3, 5], alim=am, n_samples=pr.M, profile="torque", gap_tol=1e-6,
                           tau_max=60.0, payload=held, link_ee=cfg["link_ee"])
    assert set(u) == set(ALL)
    for k in ALL:
        assert _same(u[k], want[k]), k
    want = h.retime_paths_torque(torque.plans, vm, am, n_samples=pr.M)
    u = utils.retime_plans(robot, torque.plans, alim=am, n_samples=pr.M, profile="torque")
    for k in ALL:
        assert _same(u[k], want[k]), k
    assert "tau" not in utils.retime_plans(robot, torque.plans, n_samples=pr.M, profile="convex")
    del hu
    chain.close()
    robot.close()
