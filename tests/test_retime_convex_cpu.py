"""CPU: the convex retiming's restatement (tests/retime_convex_ref.py) on the paths the greedy pass gives up on, against
the greedy profile, against scipy's SLSQP on the same rows; the header, the binding and the exported symbols of
gto_retime_paths_convex[_device]; what the Python layers refuse before they reach the library."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import retime_convex_ref as cr
import retime_paths_ref as pr
import retime_ref as rr

GAP_TOL = 1e-8
# SLSQP's own accuracy on these cases: the largest relative disagreement of its optimum (ftol 1e-15, started from the
# restatement's answer scaled by 0.99) with the restatement run at gap_tol = 1e-12, measured over all 60 paths of
# SLSQP_CASES on the CPU: 3.1e-13 (SLSQP ends up to 7e-13 outside a row, so slightly below the optimum; its success flag
# is False on 25 of the 60 and says nothing about this).  Stated with a margin of x10.
EPS_SLSQP = 3.1e-12
SLSQP_CASES = [(name, Tp, subdiv) for name in ("panda", "chain_1") for Tp in (4, 5, 11) for subdiv in (1, 2)]
# the 30 Panda paths of four columns at subdiv = 1, seed -> the paths the greedy restatement flags
FLAGGED = {0: [1], 1: [1, 4], 2: [3, 4], 3: [2, 4], 4: [0, 1, 2], 5: [2]}


@functools.lru_cache(maxsize=None)
def _both(name, Tp, mixed, subdiv, seed=None):
    """(inputs, greedy restatement, convex restatement), each computed once."""
    inp = pr.inputs(name, Tp, mixed, seed)
    _, paths, n_cols, vm, am = inp
    with np.errstate(divide="ignore", invalid="ignore"):
        greedy = pr.retime_paths_ref(paths, n_cols, vm, am, subdiv, pr.M)
        convex = cr.retime_paths_convex_ref(paths, n_cols, vm, am, subdiv, pr.M, GAP_TOL)
    return inp, greedy, convex


def _path_rows(path, vm, am, subdiv):
    moving = np.any(path != path[:, :1], axis=1)
    _, _, p1, p2 = rr.path_derivatives(path, subdiv)
    p1[:, ~moving] = 0.0
    p2[:, ~moving] = 0.0
    return cr.rows(p1, p2, np.asarray(vm, float), np.asarray(am, float), moving)


def _feasible(path, vm, am, subdiv, sd):
    A, b = _path_rows(path, vm, am, subdiv)
    x = sd ** 2
    assert x[0] == 0 and x[-1] == 0
    assert np.all(A @ x[1:-1] <= b * (1 + 1e-9) + 1e-300)


# ------------------------------------------------------------------------------------------ (a) the flagged paths
@pytest.mark.parametrize("seed", sorted(FLAGGED))
def test_paths_the_greedy_pass_flags_get_a_finite_duration(seed):
    (_, paths, _, vm, am), greedy, convex = _both("panda", 4, False, 1, seed)
    assert np.nonzero(greedy["status"] != 0)[0].tolist() == FLAGGED[seed]
    assert np.all(convex["status"] == 0) and np.all(np.isfinite(convex["duration"]))
    assert np.all(convex["duration"][FLAGGED[seed]] > 4.0) and np.all(convex["duration"][FLAGGED[seed]] < 5.7)
    for b in range(pr.B):
        _feasible(paths[b], vm, am, 1, convex["sd_grid"][b])
        assert np.all(np.isfinite(convex["q"][b])) and np.all(np.isfinite(convex["qdd"][b]))
    assert 0 < convex["iters"].max() <= cr.MAX_NEWTON // 2


def test_the_optimum_of_an_unflagged_path_can_be_much_shorter():
    _, greedy, convex = _both("panda", 4, False, 1, 0)
    assert greedy["status"][0] == 0 and abs(greedy["duration"][0] - 10.483) < 1e-3
    assert abs(convex["duration"][0] - 4.393) < 1e-3


# ------------------------------------------------------------------------------------------ (b) against the greedy profile
def _never_longer(name, Tp, mixed, subdiv):
    (_, paths, n_cols, vm, am), greedy, convex = _both(name, Tp, mixed, subdiv)
    cols = [Tp] * pr.B if n_cols is None else n_cols.tolist()
    for b, Cb in enumerate(cols):
        if Cb == 1:
            assert convex["status"][b] == 0 and convex["duration"][b] == 0 and convex["iters"][b] == 0
            continue
        if pr.unavoidable_stall(Cb, subdiv):
            assert convex["status"][b] == cr.GTO_STATUS_NUMERICAL and np.isinf(convex["duration"][b])
            continue
        assert convex["status"][b] == 0
        _feasible(paths[b][:, :Cb], vm, am, subdiv, convex["sd_grid"][b][:subdiv * (Cb - 1) + 1])
        if greedy["status"][b] == 0:  # the greedy profile is feasible, so the optimum cannot exceed it
            assert convex["duration"][b] <= greedy["duration"][b] * (1 + GAP_TOL)
    assert convex["iters"].max() <= cr.MAX_NEWTON // 2


@pytest.mark.parametrize("subdiv", pr.SUBDIVS)
@pytest.mark.parametrize("Tp", pr.TPS)
@pytest.mark.parametrize("name", pr.ROBOTS)
def test_never_longer_than_the_greedy_profile(name, Tp, subdiv):
    _never_longer(name, Tp, False, subdiv)


@pytest.mark.parametrize("subdiv", pr.SUBDIVS)
@pytest.mark.parametrize("name", pr.ROBOTS)
def test_never_longer_than_the_greedy_profile_mixed_counts(name, subdiv):
    _never_longer(name, pr.MIXED_TP, True, subdiv)


# ------------------------------------------------------------------------------------------ (c) against SLSQP
@pytest.mark.parametrize("name,Tp,subdiv", SLSQP_CASES)
def test_against_slsqp_on_the_same_rows(name, Tp, subdiv):
    from scipy.optimize import minimize
    (_, paths, _, vm, am), _, convex = _both(name, Tp, False, subdiv)
    for b in range(pr.B):
        assert convex["status"][b] == 0
        A, rhs = _path_rows(paths[b], vm, am, subdiv)
        x = convex["sd_grid"][b][1:-1] ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            res = minimize(cr.total_time, 0.99 * x, jac=lambda y: cr.time_derivatives(y)[0], method="SLSQP",
                           constraints=[dict(type="ineq", fun=lambda y: rhs - A @ y, jac=lambda y: -A)],
                           bounds=[(1e-14, None)] * len(x), options=dict(ftol=1e-15, maxiter=500))
        d = convex["duration"][b]
        assert abs(cr.total_time(x) - d) <= 1e-14 * d
        print(name, Tp, subdiv, b, "d", d, "slsqp", res.fun, "rel", (d - res.fun) / d)
        assert abs(d - res.fun) <= (GAP_TOL + EPS_SLSQP) * d


# ------------------------------------------------------------------------------------------ (d) contract and binding
@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


NEW = ("gto_retime_paths_convex", "gto_retime_paths_convex_device")


def _header_args(name):
    hdr = open(os.path.join(ROOT, "include", "gto_solver.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_binding_and_library_agree_on_the_new_entry_points(capi):
    lib = capi.load_library()
    host, dev = _header_args(NEW[0]), _header_args(NEW[1])
    assert dev[:-1] == host and dev[-1] == "void* stream"
    assert [a.split()[-1] for a in host] == ["h", "B", "Tp", "paths", "n_cols", "vmax", "amax", "subdiv", "M", "gap_tol", "max_newton",
                                            "duration_out", "t_grid_out", "sd_grid_out", "q_out", "qd_out", "qdd_out",
                                            "status_out", "iters_out"]
    old = _header_args("gto_retime_paths")
    assert host[:9] == old[:9] and host[11:18] == old[9:] and host[9:11] == ["double gap_tol", "int32_t max_newton"]
    assert host[18] == "int32_t* iters_out"
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    V, I32, D = C.c_void_p, C.c_int32, C.c_double
    assert capi.PROTOTYPES[NEW[0]] == (C.c_int, [V, I32, I32, pd, pi, pd, pd, I32, I32, D, I32, pd, pd, pd, pd, pd, pd, pi, pi])
    assert capi.PROTOTYPES[NEW[1]] == (C.c_int, [V, I32, I32, V, V, pd, pd, I32, I32, D, I32] + [V] * 9)
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == capi.PROTOTYPES[name][1]
    # a null handle is refused before anything else is looked at
    assert lib.gto_retime_paths_convex(None, 1, 4, None, None, None, None, 1, 2, 1e-8, 10, *([None] * 8)) == -1
    assert lib.gto_retime_paths_convex_device(None, 1, 4, None, None, None, None, 1, 2, 1e-8, 10, *([None] * 9)) == -1


def test_a_library_without_the_new_entry_points_is_refused_by_name(capi, tmp_path):
    import subprocess
    src = tmp_path / "old.c"
    src.write_text(f"int gto_version(void) {{ return {capi.ABI_VERSION}; }}\n")
    so = tmp_path / "libgto_old.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    with pytest.raises(RuntimeError, match="gto_retime_paths_convex"):
        capi.load_library(str(so))


def test_abi_number_stays(capi):
    hdr = open(os.path.join(ROOT, "include", "gto_solver.h")).read()
    assert int(re.search(r"#define GTO_ABI_VERSION (\d+)", hdr).group(1)) == capi.ABI_VERSION == capi.load_library().gto_version()


@pytest.mark.parametrize("kw", [dict(profile="fastest"), dict(profile=None), dict(profile="convex", gap_tol=0.0),
                                dict(profile="convex", gap_tol=-1e-8), dict(profile="convex", gap_tol=np.nan),
                                dict(profile="convex", gap_tol=np.inf), dict(profile="convex", max_newton=0)])
def test_python_layers_refuse_a_bad_profile_before_the_library(capi, kw):
    """utils.retime_plans / retime_paths and GTOPlanner.retrieve_path check the request first: no handle is made (the robot
    here has none to give), no library call."""
    from grasptrajopt_amd import utils

    class NoRobot:
        def __getattr__(self, k):
            raise AssertionError(f"the robot was asked for {k} before the profile was checked")

    with pytest.raises(ValueError, match="profile|gap_tol|max_newton"):
        capi.retime_profile(**kw)
    with pytest.raises(ValueError, match="profile|gap_tol|max_newton"):
        utils.retime_plans(NoRobot(), np.zeros((1, 9, 5)), **kw)
    with pytest.raises(ValueError, match="profile|gap_tol|max_newton"):
        utils.retime_paths(NoRobot(), np.zeros((1, 9, 5)), **kw)


def test_profile_defaults(capi):
    import inspect
    from grasptrajopt_amd import utils
    assert capi.retime_profile() == ("greedy", 1e-8, capi.RETIME_MAX_NEWTON)
    assert capi.retime_profile("convex", 1e-6, 7) == ("convex", 1e-6, 7)
    assert capi.RETIME_MAX_NEWTON == cr.MAX_NEWTON
    for fn in (utils.retime_plans, utils.retime_paths):
        p = inspect.signature(fn).parameters
        assert p["profile"].default == "greedy" and p["gap_tol"].default == 1e-8
    for m in (capi.SolverHandle.retime_paths_convex, capi.SolverHandle.retime_paths_convex_device):
        p = inspect.signature(m).parameters
        assert p["gap_tol"].default == 1e-8 and p["max_newton"].default == capi.RETIME_MAX_NEWTON
