"""gto_retime_paths without a GPU: the prototypes, the restatement of its fill rules (tests/retime_paths_ref.py), the recorded
seeds of the inputs the GPU tests use, and independent LPs on the shortest grids."""
import os
import re

import numpy as np
import pytest

from grasptrajopt_amd import _capi
import retime_paths_ref as pr
import retime_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gto_retime_paths", "gto_retime_paths_device")


def test_prototypes_in_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "gto_solver.h")).read()
    for name in NEW:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        args = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        restype, argtypes = _capi.PROTOTYPES[name]
        assert len(args) == len(argtypes) == (17 if name.endswith("_device") else 16)
        assert name in _capi.EXPORTED_SYMBOLS
    # (handle, B, Tp, paths, n_cols, vmax, amax, subdiv, M, seven outputs[, stream]); additions: the ABI number stays
    dev = _capi.PROTOTYPES["gto_retime_paths_device"][1]
    batch = _capi.PROTOTYPES["gto_retime_batch_device"][1]
    assert dev[:2] == batch[:2] and dev[5:] == batch[3:]
    assert int(re.search(r"#define GTO_ABI_VERSION (\d+)", hdr).group(1)) == _capi.ABI_VERSION
    assert callable(_capi.SolverHandle.retime_paths) and callable(_capi.SolverHandle.retime_paths_device)


def test_python_surface_signatures():
    import inspect
    from grasptrajopt_amd import utils
    from grasptrajopt_amd.gto_planner import GTOPlanner
    from grasptrajopt_amd.grasp_chain import GraspChain
    assert list(inspect.signature(utils.retime_paths).parameters)[:5] == ["robot", "paths", "n_cols", "vlim", "alim"]
    assert inspect.signature(GTOPlanner.retrieve_path).parameters["retime"].default is None
    assert "not retimed" not in GTOPlanner.retrieve_path.__doc__ and "not retimed" not in GraspChain.plan_objects.__doc__
    sh = inspect.signature(_capi.SolverHandle.retime_paths).parameters
    assert list(sh)[1:5] == ["paths", "vmax", "amax", "n_cols"] and sh["subdiv"].default == 2 and sh["n_samples"].default == 100


def test_fill_rules_of_the_restatement():
    desc, paths, n_cols, vm, am = pr.inputs("panda", pr.MIXED_TP, mixed=True)
    for subdiv in pr.SUBDIVS:
        r = pr.retime_paths_ref(paths, n_cols, vm, am, subdiv, pr.M)
        Nmax = subdiv * (pr.MIXED_TP - 1) + 1
        assert r["t_grid"].shape == r["sd_grid"].shape == (pr.B, Nmax)
        for b, C in enumerate(pr.MIXED_COLS):
            N = subdiv * (C - 1) + 1
            one = rr.retime_one(paths[b][:, :C], vm, am, subdiv, pr.M) if C > 1 else None
            assert np.all(r["t_grid"][b, N:] == r["duration"][b]) and np.all(r["sd_grid"][b, N:] == 0)
            if C == 1:  # the stationary rule
                assert r["status"][b] == 0 and r["duration"][b] == 0 and np.all(r["t_grid"][b] == 0)
                assert np.all(r["q"][b] == paths[b][:, 0]) and np.all(r["qd"][b] == 0) and np.all(r["qdd"][b] == 0)
            else:
                assert np.array_equal(r["t_grid"][b, :N], one["t_grid"]) and np.array_equal(r["sd_grid"][b, :N], one["sd_grid"])
                assert np.array_equal(r["q"][b], one["q"], equal_nan=True) and r["status"][b] == one["status"]
    # a count outside [1, Tp], and a non-finite value inside the used columns: NaN over all of Nmax; outside them: ignored
    bad = paths.copy()
    bad[4, 2, 5] = np.nan   # C = 11: used
    bad[2, 2, 5] = np.nan   # C = 3: not used
    clean = pr.retime_paths_ref(paths, n_cols, vm, am, 2, pr.M)
    for cols in ([1, 0, 3, 4, 11], [1, -1, 3, 4, 11], [1, 12, 3, 4, 11]):
        r = pr.retime_paths_ref(bad, cols, vm, am, 2, pr.M)
        for b in (1, 4):
            assert r["status"][b] == rr.GTO_STATUS_NUMERICAL and np.isnan(r["duration"][b])
            assert np.all(np.isnan(r["t_grid"][b])) and np.all(np.isnan(r["sd_grid"][b])) and np.all(np.isnan(r["q"][b]))
        for b in (0, 2, 3):
            for k in r:
                assert np.array_equal(r[k][b], clean[k][b], equal_nan=True), (k, b)


@pytest.mark.parametrize("name", pr.ROBOTS)
def test_recorded_seeds_converge(name):
    """Every path of two columns or more that the GPU tests compare has a converged restatement -- but for N = 2 (two columns
    at subdiv = 1), where both gridpoints are ends at rest and the duration is infinite by construction."""
    for Tp in pr.TPS:
        assert pr.flagged(name, Tp) == [], Tp
    assert pr.flagged(name, pr.MIXED_TP, mixed=True) == []
    desc, paths, _, vm, am = pr.inputs(name, 2)
    with np.errstate(divide="ignore"):
        r = pr.retime_paths_ref(paths, None, vm, am, 1, pr.M)
    assert pr.unavoidable_stall(2, 1) and not pr.unavoidable_stall(2, 2) and not pr.unavoidable_stall(3, 1)
    assert np.all(r["status"] == rr.GTO_STATUS_NUMERICAL) and np.all(np.isinf(r["duration"])) and np.all(r["sd_grid"] == 0)


@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("subdiv", [2, 3])
def test_grid_lp_admits_the_profile_on_the_shortest_paths(C, subdiv):
    """The restatement's profile of a path of 2, 3 and 4 columns satisfies the grid constraints as an independent LP states
    them: it is feasible (the limits hold at every gridpoint) and its sum of x is at most the LP's optimum."""
    desc, paths, _, vm, am = pr.inputs("panda", C)
    for b in range(pr.B):
        r = rr.retime_one(paths[b], vm, am, subdiv, pr.M)
        assert r["status"] == 0
        moving = np.any(paths[b] != paths[b][:, :1], axis=1)
        _, _, p1, p2 = rr.path_derivatives(paths[b], subdiv)
        p1[:, ~moving] = 0.0
        p2[:, ~moving] = 0.0
        if C == 2:
            assert np.all(p2 == 0.0)   # scipy's spline through two points is the straight line
        x = r["sd_grid"] ** 2
        N = x.shape[0]
        u = (x[1:] - x[:-1]) * 0.5 * (N - 1)
        assert np.all(np.abs(p1[:-1] * u[:, None] + p2[:-1] * x[:-1, None]) <= am * (1 + 1e-9))
        fin = np.isfinite(vm)
        assert np.all(np.abs(p1[:, fin]) * r["sd_grid"][:, None] <= vm[fin] * (1 + 1e-9))
        x_lp = rr.grid_lp(p1, p2, vm, am)
        assert x[0] == 0 and x[-1] == 0 and x.sum() > 0
        assert x.sum() <= x_lp.sum() * (1 + 1e-9)
        assert np.all(x <= np.array([rr.controllable_lp(p1, p2, vm, am, i) for i in range(N)]) * (1 + 1e-7) + 1e-15)
