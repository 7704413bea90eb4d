"""GPU: gto_retime_paths_convex[_device] against the restatement (tests/retime_convex_ref.py), against limits, times and
samples recomputed from its own outputs, against the greedy call on the same inputs, under batching and padding, at the
edges of the contract, and through the Python layers.  Every call goes through the C ABI.

Durations: the GPU's profile and the restatement's are both feasible and both certified, so both lie in
[T*, (1 + gap_tol) T*]: |d_gpu - d_ref| <= gap_tol d_ref, with (1 + RTOL) for the round-off of the sums."""
import functools

import numpy as np
import pytest

from grasptrajopt_amd import _capi
import retime_convex_ref as cr
import retime_paths_ref as pr
import retime_ref as rr
from test_gpu_retime import KEYS, LIMIT_SLACK, PATH_ATOL, RTOL, _close, _limit_handle, _moving_plans, _same, _wide_limits

pytestmark = pytest.mark.gpu
ALL = KEYS + ("status", "iters")
GAP_TOL = 1e-8
NUMERICAL, MAX_ITER = cr.GTO_STATUS_NUMERICAL, cr.GTO_STATUS_MAX_ITER
FLAGGED_SEEDS = (0, 1, 2, 3, 4, 5)   # retime_paths_ref.inputs("panda", 4, seed=s): the greedy pass flags 11 of the 30 paths


@pytest.fixture(scope="module")
def handles():
    """name -> (desc, handle): the Panda at T = 50, small_robots' one-joint chain at T = 5."""
    import json
    import os
    import small_robots as sr
    from grasptrajopt_amd.robot_desc import load_builtin
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = json.load(open(os.path.join(root, "grasptrajopt_amd", "data", "panda_cfg.json")))
    o = _capi.default_opts()
    o.T = 50
    made = {"panda": (load_builtin("panda"), _capi.SolverHandle(load_builtin("panda"), cfg["link_ee"], cfg["link_gripper"], o, device=0))}
    r = sr.Robot("chain_1")
    o = _capi.default_opts()
    o.T, o.standoff_offset = 5, sr.HORIZONS[5]
    made["chain_1"] = (r.desc, _capi.SolverHandle(r.desc, r.ee, r.gripper, o, device=0, n_gripper_points=r.n_gripper_points))
    yield made
    for _, h in made.values():
        h.close()


@functools.lru_cache(maxsize=None)
def _reference(name, Tp, mixed, subdiv, seed=None):
    _, paths, n_cols, vm, am = pr.inputs(name, Tp, mixed, seed)
    with np.errstate(divide="ignore", invalid="ignore"):
        return cr.retime_paths_convex_ref(paths, n_cols, vm, am, subdiv, pr.M, GAP_TOL)


def _recomputed(paths, cols, g, vm, am, subdiv, M):
    """Feasibility, times and samples from the outputs alone: p1 and p2 from scipy's spline, every velocity and acceleration
    row within LIMIT_SLACK, both ends at rest, t_grid the cumulative segment times of sd_grid, the samples those of the
    restatement's sampling code on the GPU's own profile."""
    vm, am = np.asarray(vm, float), np.asarray(am, float)
    for b, C in enumerate(cols):
        N = subdiv * (C - 1) + 1
        if g["status"][b] == NUMERICAL or N < 3:
            continue
        used = paths[b][:, :C]
        moving = np.any(used != used[:, :1], axis=1)
        if not moving.any():
            continue
        _, _, p1, p2 = rr.path_derivatives(used, subdiv)
        p1[:, ~moving] = 0.0
        p2[:, ~moving] = 0.0
        sd, t = g["sd_grid"][b][:N], g["t_grid"][b][:N]
        x = sd ** 2
        u = (x[1:] - x[:-1]) * 0.5 * (N - 1)
        fin = np.isfinite(vm)
        assert sd[0] == 0 and sd[-1] == 0 and np.all(sd[1:-1] > 0)
        assert np.all(np.abs(p1[:, fin]) * sd[:, None] <= vm[fin] * (1 + LIMIT_SLACK) + 1e-300)
        assert np.all(np.abs(p1[:-1] * u[:, None] + p2[:-1] * x[:-1, None]) <= am * (1 + LIMIT_SLACK))
        want_t = np.concatenate([[0.0], np.cumsum((2.0 / (N - 1)) / (sd[:-1] + sd[1:]))])
        _close(t, want_t)
        assert g["duration"][b] == t[-1]
        r = cr.sample(used, x, subdiv, M)
        _close(g["q"][b], r["q"])
        _close(g["qd"][b], r["qd"])
        ts = np.linspace(0, r["duration"], M)
        far = np.abs(ts[:, None] - r["t_grid"][None, 1:-1]).min(axis=1, initial=np.inf) > 1e-9 * r["duration"]
        _close(g["qdd"][b][far], r["qdd"][far])
        np.testing.assert_allclose(g["q"][b][0], used[:, 0], rtol=0, atol=PATH_ATOL)
        np.testing.assert_allclose(g["q"][b][-1], used[:, -1], rtol=0, atol=PATH_ATOL)


def _against_reference_and_greedy(h, paths, n_cols, vm, am, subdiv, r, M=pr.M):
    """The convex call between two greedy calls on the same inputs: durations against the restatement's, never longer
    than the greedy profile where that converged, and the greedy outputs bit-equal before and after.  A path on which no
    joint moves has nothing to solve: duration 0, no Newton step, every sample the waypoint, as the restatement has it."""
    B, _, Tp = paths.shape
    cols = [Tp] * B if n_cols is None else [int(c) for c in n_cols]
    before = h.retime_paths(paths, vm, am, n_cols=n_cols, subdiv=subdiv, n_samples=M)
    g = h.retime_paths_convex(paths, vm, am, n_cols=n_cols, subdiv=subdiv, n_samples=M, gap_tol=GAP_TOL)
    after = h.retime_paths(paths, vm, am, n_cols=n_cols, subdiv=subdiv, n_samples=M)
    for k in KEYS + ("status",):
        assert _same(before[k], after[k]), k
    assert g["t_grid"].shape == (B, subdiv * (Tp - 1) + 1) and g["iters"].dtype == np.int32
    assert np.array_equal(g["status"], r["status"])
    for b, C in enumerate(cols):
        N = subdiv * (C - 1) + 1
        gt, gs = g["t_grid"][b], g["sd_grid"][b]
        assert _same(gt[N:], np.full(len(gt) - N, g["duration"][b])) and _same(gs[N:], np.zeros(len(gs) - N))
        if C == 1:
            assert g["status"][b] == 0 and g["duration"][b] == 0 and g["iters"][b] == 0 and _same(gt, np.zeros(len(gt)))
            assert _same(g["q"][b], r["q"][b]) and _same(g["qd"][b], r["qd"][b]) and _same(g["qdd"][b], r["qdd"][b])
            continue
        if not np.any(paths[b][:, :C] != paths[b][:, :1]):  # nothing moves
            assert g["status"][b] == 0 and g["duration"][b] == 0 and g["iters"][b] == 0 and r["duration"][b] == 0 and r["iters"][b] == 0
            assert np.all(gt == 0) and np.all(gs == 0) and np.all(g["q"][b] == paths[b][:, 0]) and np.all(g["q"][b] == r["q"][b])
            assert np.all(g["qd"][b] == 0) and np.all(g["qdd"][b] == 0)
            continue
        if pr.unavoidable_stall(C, subdiv):  # N = 2: no variable
            assert g["status"][b] == NUMERICAL and np.isinf(g["duration"][b]) and _same(gs, np.zeros(len(gs)))
            assert np.all(np.isnan(g["q"][b])) and g["iters"][b] == 0
            continue
        assert g["status"][b] == 0 and 0 < g["iters"][b] <= _capi.RETIME_MAX_NEWTON // 2
        d_gpu, d_ref = g["duration"][b], r["duration"][b]
        print(f"b {b} C {C} subdiv {subdiv}: d_gpu {d_gpu!r} d_ref {d_ref!r} iters {g['iters'][b]} / {r['iters'][b]} greedy {before['duration'][b]!r}")
        assert abs(d_gpu - d_ref) <= GAP_TOL * d_ref * (1 + RTOL)
        if before["status"][b] == 0:
            assert d_gpu <= before["duration"][b] * (1 + GAP_TOL)
    _recomputed(paths, cols, g, vm, am, subdiv, M)
    return g


# ------------------------------------------------------------------------------------------ 1. durations, feasibility, greedy
@pytest.mark.parametrize("subdiv", pr.SUBDIVS)
@pytest.mark.parametrize("Tp", pr.TPS)
@pytest.mark.parametrize("name", pr.ROBOTS)
def test_every_column_used(handles, name, Tp, subdiv):
    _, h = handles[name]
    _, paths, _, vm, am = pr.inputs(name, Tp)
    _against_reference_and_greedy(h, paths, None, vm, am, subdiv, _reference(name, Tp, False, subdiv))


@pytest.mark.parametrize("subdiv", pr.SUBDIVS)
@pytest.mark.parametrize("name", pr.ROBOTS)
def test_mixed_counts(handles, name, subdiv):
    _, h = handles[name]
    _, paths, n_cols, vm, am = pr.inputs(name, pr.MIXED_TP, mixed=True)
    g = _against_reference_and_greedy(h, paths, n_cols, vm, am, subdiv, _reference(name, pr.MIXED_TP, True, subdiv))
    assert g["status"].tolist() == [0, NUMERICAL if subdiv == 1 else 0, 0, 0, 0]


@pytest.mark.parametrize("seed", FLAGGED_SEEDS)
def test_paths_the_greedy_pass_flags(handles, seed):
    _, h = handles["panda"]
    _, paths, _, vm, am = pr.inputs("panda", 4, seed=seed)
    greedy = h.retime_paths(paths, vm, am, subdiv=1, n_samples=pr.M)
    g = _against_reference_and_greedy(h, paths, None, vm, am, 1, _reference("panda", 4, False, 1, seed))
    flagged = greedy["status"] != 0
    assert flagged.any() and np.all(g["status"] == 0) and np.all(np.isfinite(g["q"]))
    assert np.all(g["duration"][flagged] > 4.0) and np.all(g["duration"][flagged] < 5.7)


# ------------------------------------------------------------------------------------------ 2. batch, position, padding
def _device_call(h, desc, paths, n_cols, lim, subdiv=2, M=pr.M, gap_tol=GAP_TOL, max_newton=_capi.RETIME_MAX_NEWTON):
    """gto_retime_paths_convex_device on a side stream, every output prefilled."""
    import torch
    B, _, Tp = paths.shape
    N = subdiv * (Tp - 1) + 1
    dev = "cuda:0"
    f64 = dict(dtype=torch.float64, device=dev)
    out = dict(duration=torch.full((B,), -7.0, **f64), t_grid=torch.full((B, N), -7.0, **f64), sd_grid=torch.full((B, N), -7.0, **f64),
               q=torch.full((B, M, desc.ndof), -7.0, **f64), qd=torch.full((B, M, desc.ndof), -7.0, **f64),
               qdd=torch.full((B, M, desc.ndof), -7.0, **f64), status=torch.full((B,), -7, dtype=torch.int32, device=dev),
               iters=torch.full((B,), -7, dtype=torch.int32, device=dev))
    Pd = torch.from_numpy(np.ascontiguousarray(paths)).to(dev)
    nc = None if n_cols is None else torch.from_numpy(np.ascontiguousarray(n_cols, dtype=np.int32)).to(dev)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    h.retime_paths_convex_device(B, Tp, Pd.data_ptr(), *lim, None if nc is None else nc.data_ptr(), subdiv, M, gap_tol, max_newton,
                                 *(out[k].data_ptr() for k in ALL), stream=st.cuda_stream)
    st.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_batch_position_and_padding_do_not_change_a_bit(handles):
    desc, h = handles["panda"]
    _, paths, _, vm, am = pr.inputs("panda", 11, batch=9)
    cols = np.array([11, 3, 7, 2, 5, 9, 1, 4, 11], dtype=np.int32)
    for subdiv in pr.SUBDIVS:
        whole = _device_call(h, desc, paths, cols, (vm, am), subdiv)
        host = h.retime_paths_convex(paths, vm, am, n_cols=cols, subdiv=subdiv, n_samples=pr.M)
        back = _device_call(h, desc, paths[::-1], cols[::-1], (vm, am), subdiv)
        wide = np.full((9, desc.ndof, 19), np.nan)
        wide[:, :, :11] = paths
        padded = _device_call(h, desc, wide, cols, (vm, am), subdiv)
        assert (whole["status"] == 0).sum() >= (8 if subdiv == 2 else 7)
        for k in ALL:
            assert _same(whole[k], host[k]) and _same(whole[k], back[k][::-1]), k
        N11 = subdiv * 10 + 1
        for k in ("duration", "q", "qd", "qdd", "status", "iters"):
            assert _same(whole[k], padded[k]), k
        assert _same(padded["t_grid"][:, :N11], whole["t_grid"]) and _same(padded["sd_grid"][:, :N11], whole["sd_grid"])
        assert _same(padded["t_grid"][:, N11:], np.repeat(whole["duration"][:, None], padded["t_grid"].shape[1] - N11, axis=1))
        assert _same(padded["sd_grid"][:, N11:], np.zeros((9, padded["sd_grid"].shape[1] - N11)))
        for b in range(9):
            one = _device_call(h, desc, paths[b:b + 1], cols[b:b + 1], (vm, am), subdiv)
            for k in ALL:
                assert _same(one[k][0], whole[k][b]), (k, b)


# ------------------------------------------------------------------------------------------ 3. edges
def test_one_variable(handles):
    """N = 3: three columns at subdiv 1, two at subdiv 2."""
    for name in pr.ROBOTS:
        desc, h = handles[name]
        for Tp, subdiv in ((3, 1), (2, 2)):
            _, paths, _, vm, am = pr.inputs(name, Tp)
            g = h.retime_paths_convex(paths, vm, am, subdiv=subdiv, n_samples=pr.M)
            assert g["t_grid"].shape == (pr.B, 3) and np.all(g["status"] == 0) and np.all(g["iters"] > 0)
            assert np.all(g["sd_grid"][:, 1] > 0) and _same(g["duration"], g["t_grid"][:, 2])


@pytest.mark.parametrize("Tp,subdiv", [(1024, 1), (342, 3)])
def test_the_longest_grid_on_the_widest_robot(Tp, subdiv):
    """N = 1024 gridpoints, the most the kernel's LDS arrays and trip counts are sized for, B = 3, on the chain with 16
    optimised joints of tests/helpers.limit_robot (31 joints, all moving: 62 acceleration rows per gridpoint)."""
    desc, h = _limit_handle(50)
    paths = _moving_plans(desc, 3, Tp, np.arange(31), seed=Tp)
    vm, am = _wide_limits(desc)
    greedy = h.retime_paths(paths, vm, am, subdiv=subdiv, n_samples=pr.M)
    g = h.retime_paths_convex(paths, vm, am, subdiv=subdiv, n_samples=pr.M)
    print("iters", g["iters"], "durations", g["duration"], "greedy", greedy["duration"], greedy["status"])
    assert g["sd_grid"].shape == (3, 1024) and np.all(g["status"] == 0)
    assert np.all(g["iters"] > 0) and np.all(g["iters"] <= _capi.RETIME_MAX_NEWTON // 2)
    ok = greedy["status"] == 0
    assert np.all(g["duration"][ok] <= greedy["duration"][ok] * (1 + GAP_TOL))
    _recomputed(paths, [Tp] * 3, g, vm, am, subdiv, pr.M)
    h.close()


def test_one_moving_joint_none_and_a_joint_without_a_line():
    desc, h = _limit_handle(50)
    vm, am = _wide_limits(desc)
    # one moving joint, and none: duration 0, no Newton step, every sample the waypoint
    paths = np.concatenate([_moving_plans(desc, 2, 50, np.array([15]), seed=1), _moving_plans(desc, 1, 50, np.array([], dtype=int), seed=2)])
    g = h.retime_paths_convex(paths, vm, am, n_samples=pr.M)
    r = cr.retime_paths_convex_ref(paths[:2], None, vm, am, 2, pr.M, GAP_TOL)
    assert g["status"].tolist() == [0, 0, 0] and g["iters"][2] == 0 and np.all(g["iters"][:2] > 0)
    assert np.all(np.abs(g["duration"][:2] - r["duration"]) <= GAP_TOL * r["duration"] * (1 + RTOL))
    assert g["duration"][2] == 0 and np.all(g["t_grid"][2] == 0) and np.all(g["sd_grid"][2] == 0)
    assert np.all(g["q"][2] == paths[2, :, 0]) and np.all(g["qd"][2] == 0) and np.all(g["qdd"][2] == 0)
    _recomputed(paths, [50] * 3, g, vm, am, 2, pr.M)
    # the joint that moves by 1e-300 under a large acceleration limit has no line: it bounds x through xcap alone
    paths = _moving_plans(desc, 4, 50, np.arange(31), seed=9)
    s = np.linspace(0.0, 1.0, 50)
    paths[:, 12] = 1e-300 * (3 * s ** 2 - 2 * s ** 3)[None] * np.array([1.0, -2.0, 0.5, 3.0])[:, None]
    am = am.copy()
    am[12] = 1e12
    for b in range(4):
        _, _, p1, p2 = rr.path_derivatives(paths[b], 2)
        assert np.any(p1[:, 12] != 0) and not rr._has_line(p1[:, 12], p2[:, 12], np.full(len(p1), am[12])).any()
    g = h.retime_paths_convex(paths, vm, am, n_samples=pr.M)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = cr.retime_paths_convex_ref(paths, None, vm, am, 2, pr.M, GAP_TOL)
    assert np.all(g["status"] == 0) and np.all(r["status"] == 0)
    assert np.all(np.abs(g["duration"] - r["duration"]) <= GAP_TOL * r["duration"] * (1 + RTOL))
    _recomputed(paths, [50] * 4, g, vm, am, 2, pr.M)
    still = paths.copy()
    still[:, 12] = 0.0
    g0 = h.retime_paths_convex(still, vm, am, n_samples=pr.M)
    assert np.all(g0["status"] == 0) and np.all(np.abs(g["duration"] - g0["duration"]) <= GAP_TOL * g0["duration"] * (1 + RTOL))
    h.close()


def test_the_newton_cap_leaves_a_feasible_profile_with_samples(handles):
    desc, h = handles["panda"]
    _, paths, n_cols, vm, am = pr.inputs("panda", pr.MIXED_TP, mixed=True)
    full = h.retime_paths_convex(paths, vm, am, n_cols=n_cols, n_samples=pr.M)
    g = h.retime_paths_convex(paths, vm, am, n_cols=n_cols, n_samples=pr.M, max_newton=1)
    assert g["status"].tolist() == [0, MAX_ITER, MAX_ITER, MAX_ITER, MAX_ITER] and g["iters"].tolist() == [0, 1, 1, 1, 1]
    assert np.all(np.isfinite(g["q"])) and np.all(np.isfinite(g["qd"])) and np.all(np.isfinite(g["qdd"]))
    assert np.all(g["duration"][1:] > full["duration"][1:])
    _recomputed(paths, n_cols, g, vm, am, 2, pr.M)
    capped = h.retime_paths_convex(paths, vm, am, n_cols=n_cols, n_samples=pr.M, max_newton=int(full["iters"].max()))
    for k in ALL:
        assert _same(capped[k], full[k]), k


@pytest.mark.parametrize("count", [0, -1, 12, 2 ** 31 - 1, -2 ** 31])
def test_a_wild_count_on_the_device_is_numerical_and_leaves_the_neighbours(handles, count):
    desc, h = handles["panda"]
    _, paths, n_cols, vm, am = pr.inputs("panda", pr.MIXED_TP, mixed=True)
    clean = _device_call(h, desc, paths, n_cols, (vm, am))
    for pos in (0, 2, 4):
        c = n_cols.copy()
        c[pos] = count
        g = _device_call(h, desc, paths, c, (vm, am))
        assert g["status"][pos] == NUMERICAL and g["iters"][pos] == 0
        for k in KEYS:
            assert np.all(np.isnan(g[k][pos])), k
        keep = np.arange(pr.B) != pos
        for k in ALL:
            assert _same(g[k][keep], clean[k][keep]), (k, pos)
        if count in (0, -1, 12):
            with pytest.raises(_capi.GTOError, match=r"\(-1\): gto_retime_paths_convex: n_cols must lie in \[1, Tp\]"):
                h.retime_paths_convex(paths, vm, am, n_cols=c)


def test_a_non_finite_value_counts_only_inside_the_used_columns(handles):
    desc, h = handles["panda"]
    _, paths, n_cols, vm, am = pr.inputs("panda", pr.MIXED_TP, mixed=True)
    clean = h.retime_paths_convex(paths, vm, am, n_cols=n_cols)
    bad = paths.copy()
    bad[2, 3, 2] = np.inf   # C = 3: the last used column
    bad[3, 3, 4] = np.nan   # C = 4: the first unused one
    bad[0, 0, 1:] = np.nan  # C = 1
    bad[4, 6, 0] = -np.inf  # C = 11: the first column
    g = h.retime_paths_convex(bad, vm, am, n_cols=n_cols)
    assert g["status"].tolist() == [0, 0, NUMERICAL, 0, NUMERICAL] and g["iters"][[2, 4]].tolist() == [0, 0]
    for k in KEYS:
        assert np.all(np.isnan(g[k][[2, 4]])), k
    for k in ALL:
        assert _same(g[k][[0, 1, 3]], clean[k][[0, 1, 3]]), k


def test_argument_checks(handles):
    desc, h = handles["panda"]
    vm, am = pr.limits("panda", desc)
    z = lambda Tp, B=1: np.zeros((B, desc.ndof, Tp))
    with pytest.raises(_capi.GTOError, match=r"\(-1\): gto_retime_paths_convex: Tp must be >= 2"):
        h.retime_paths_convex(z(1, 2), vm, am)
    h.retime_paths_convex(z(1024), vm, am, subdiv=1, n_samples=2)
    for Tp, subdiv in ((1025, 1), (513, 2), (5, 256)):
        with pytest.raises(_capi.GTOError, match=r"\(-1\): gto_retime_paths_convex: subdiv \(Tp-1\) \+ 1 must be <= 1024"):
            h.retime_paths_convex(z(Tp), vm, am, subdiv=subdiv)
    for kw in (dict(subdiv=0), dict(n_samples=1), dict(max_newton=0), dict(max_newton=-3)):
        with pytest.raises(_capi.GTOError, match=r"\(-1\)"):
            h.retime_paths_convex(z(5), vm, am, **kw)
    for tol in (0.0, -1e-8, np.nan, np.inf, -np.inf):
        with pytest.raises(_capi.GTOError, match=r"\(-1\): gto_retime_paths_convex: gap_tol must be finite and > 0"):
            h.retime_paths_convex(z(5), vm, am, gap_tol=tol)
        with pytest.raises(_capi.GTOError, match=r"\(-1\): gto_retime_paths_convex: gap_tol must be finite and > 0"):
            h.retime_paths_convex_device(0, 5, None, vm, am, gap_tol=tol)
    for lim in ((vm, -am), (vm, am * np.inf), (0 * vm, am), (vm * np.nan, am)):
        with pytest.raises(_capi.GTOError, match=r"\(-1\)"):
            h.retime_paths_convex(z(5), *lim)
    g = h.retime_paths_convex(np.empty((0, desc.ndof, 11)), vm, am, n_samples=pr.M)
    assert g["duration"].shape == (0,) and g["t_grid"].shape == (0, 21) and g["iters"].shape == (0,)
    h.retime_paths_convex_device(0, 11, None, vm, am)
    with pytest.raises(_capi.GTOError, match=r"\(-1\): gto_retime_paths_convex: null paths"):
        h.retime_paths_convex_device(1, 11, None, vm, am)
    with pytest.raises(_capi.GTOError, match=r"\(-1\)"):
        h.retime_paths_convex_device(-1, 11, None, vm, am)
    # iters_out and every other output may be NULL
    g = h.retime_paths_convex(pr.inputs("panda", 5)[1], vm, am, n_samples=pr.M)
    import torch
    Pd = torch.from_numpy(pr.inputs("panda", 5)[1]).to("cuda:0")
    dur = torch.empty(pr.B, dtype=torch.float64, device="cuda:0")
    h.retime_paths_convex_device(pr.B, 5, Pd.data_ptr(), vm, am, n_samples=pr.M, duration_out=dur.data_ptr(),
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _same(dur.cpu().numpy(), g["duration"])


# ------------------------------------------------------------------------------------------ 4. the Python layers
def test_chain_planner_and_utils_go_through_the_convex_entry():
    import grasptrajopt_amd as g
    from grasptrajopt_amd import utils
    from grasptrajopt_amd.grasp_chain import GraspChain
    from test_gpu_grasp_chain import chain_setup
    B, n = 2, 3
    cfg, robot, fields, RT = chain_setup("panda", B * n, seed=21)
    RT = RT.reshape(B, n, 4, 4)
    qc = np.array(cfg["default_pose"], dtype=np.float64)
    base = np.array([0.01, -0.02, 0.0])
    chain = GraspChain(robot, cfg["link_ee"], cfg["link_gripper"])
    chain.max_iter = 20
    vm, am = robot.desc.velocity, np.full(robot.ndof, 0.5)
    rt = dict(vmax=vm, amax=am, n_samples=pr.M)
    args, kw = (qc, RT, RT, [n, n], fields[0], base), dict(axis_standoff=cfg["axis_standoff"])
    h = chain._handle
    lift = dict(mode="lift", distance=0.1, steps=4)
    plain = chain.plan_objects(*args, retrieve=lift, retime=rt, **kw)
    named = chain.plan_objects(*args, retrieve=lift, retime=dict(rt, profile="greedy"), **kw)
    convex = chain.plan_objects(*args, retrieve=lift, retime=dict(rt, profile="convex", retrieve_samples=True), **kw)
    # without the key: the greedy calls, the keys of before
    assert set(vars(plain)) == set(vars(named)) and not any("iters" in k and "retime" in k for k in vars(plain))
    want = h.retime_batch(plain.plans, vm, am, n_samples=pr.M)
    assert _same(plain.durations, want["duration"]) and _same(plain.retime_status, want["status"])
    want = h.retime_paths(plain.retrieve_path, vm, am, n_samples=pr.M)
    assert _same(plain.retrieve_durations, want["duration"]) and _same(plain.retrieve_retime_status, want["status"])
    for k, v in vars(plain).items():
        assert _same(v, getattr(named, k)), k
    # with it: what stands in front of the retiming is unchanged, both retimings are the library's convex call
    extra = {"retime_iters", "retrieve_retime_iters", "retrieve_q", "retrieve_qd", "retrieve_qdd"}
    assert set(vars(convex)) == set(vars(plain)) | extra
    for k, v in vars(plain).items():
        if "duration" not in k and "retime" not in k:
            assert _same(v, getattr(convex, k)), k
    want = h.retime_paths_convex(convex.plans, vm, am, n_samples=pr.M)
    assert _same(convex.durations, want["duration"]) and _same(convex.retime_status, want["status"])
    assert _same(convex.retime_iters, want["iters"]) and np.all(want["status"] == 0)
    assert np.all(convex.durations <= plain.durations * (1 + GAP_TOL))
    want = h.retime_paths_convex(convex.retrieve_path, vm, am, n_samples=pr.M)
    assert _same(convex.retrieve_durations, want["duration"]) and _same(convex.retrieve_retime_status, want["status"])
    assert _same(convex.retrieve_retime_iters, want["iters"]) and np.all(want["status"] == 0)
    for k in ("q", "qd", "qdd"):
        assert _same(getattr(convex, "retrieve_" + k), want[k]), k
    loose = chain.plan_objects(*args, retime=dict(rt, profile="convex", gap_tol=1e-3, max_newton=500), **kw)
    want = h.retime_paths_convex(loose.plans, vm, am, n_samples=pr.M, gap_tol=1e-3, max_newton=500)
    assert _same(loose.durations, want["duration"]) and np.all(loose.retime_iters < convex.retime_iters)
    with pytest.raises(ValueError, match="profile"):
        chain.plan_objects(*args, retime=dict(rt, profile="fastest"), **kw)
    with pytest.raises(ValueError, match="gap_tol"):
        chain.plan_objects(*args, retime=dict(rt, profile="convex", gap_tol=0.0), **kw)
    # GTOPlanner.retrieve_path and utils
    planner = g.GTOPlanner(robot, cfg["link_ee"], cfg["link_gripper"])
    path, reached, traj = planner.retrieve_path(convex.plans[0], "lift", distance=0.1, steps=4, retime=dict(rt, profile="convex"))
    assert _same(path, convex.retrieve_path[0]) and traj["duration"] == convex.retrieve_durations[0]
    assert traj["iters"] == convex.retrieve_retime_iters[0] and _same(traj["q"], convex.retrieve_q[0])
    path, reached, old = planner.retrieve_path(convex.plans[0], "lift", distance=0.1, steps=4, retime=rt)
    assert "iters" not in old and old["duration"] == plain.retrieve_durations[0]
    with pytest.raises(ValueError, match="gap_tol"):
        planner.retrieve_path(convex.plans[0], "lift", distance=0.1, steps=4, retime=dict(rt, profile="convex", gap_tol=np.nan))
    with pytest.raises(TypeError):
        planner.retrieve_path(convex.plans[0], "lift", distance=0.1, steps=4, retime=dict(rt, speed=1))
    want = h.retime_paths_convex(convex.retrieve_path, vm, am, n_cols=[3, 5], n_samples=pr.M, gap_tol=1e-6)
    u = utils.retime_paths(robot, convex.retrieve_path, n_cols=[3, 5], n_samples=pr.M, profile="convex", gap_tol=1e-6)
    assert set(u) == set(ALL)
    for k in ALL:
        assert _same(u[k], want[k]), k
    want = h.retime_paths_convex(convex.plans, vm, am, n_samples=pr.M)
    u = utils.retime_plans(robot, convex.plans, n_samples=pr.M, profile="convex")
    for k in ALL:
        assert _same(u[k], want[k]), k
    assert "iters" not in utils.retime_plans(robot, convex.plans, n_samples=pr.M)
    chain.close()
    robot.close()
