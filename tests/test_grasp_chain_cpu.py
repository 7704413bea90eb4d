"""CPU: the stream-ordered grasp chain's entry points exist (header, exports, ABI 1012) and validate before any device
work; the numpy restatement the GPU tests compare against (tests/grasp_chain_ref.py) is itself pinned to np.lexsort,
utils.interpolate_waypoints and the seed construction of GTOPlanner.plan_goalset."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import grasp_chain_ref as ref
from conftest import ROOT

NEW = ("gto_solve_ik_pose_batch_device", "gto_ik_report_device", "gto_seed_goalsets_device")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


def test_symbols_are_exported_declared_and_abi_is_1012(capi):
    hdr = open(os.path.join(ROOT, "include", "gto_solver.h")).read()
    assert int(re.search(r"#define GTO_ABI_VERSION (\d+)", hdr).group(1)) == 1012 == capi.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = capi.load_library()
    assert lib.gto_version() == 1012
    for sym in NEW:
        assert re.search(rf"\bint {sym}\s*\(", code), sym
        assert sym in capi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    for m in ("solve_ik_pose_batch_device", "ik_report_device", "seed_goalsets_device"):
        assert callable(getattr(capi.SolverHandle, m))


def test_null_handle_is_invalid_arg(capi):
    lib = capi.load_library()
    z = None
    assert lib.gto_solve_ik_pose_batch_device(None, 0, 1, z, z, z, z, 50, z, z, z, z, z) == -1
    assert lib.gto_ik_report_device(None, 1, z, z, z, z, 0.01, 5.0, 5.0, z, z, z, z, z) == -1
    assert lib.gto_seed_goalsets_device(None, 1, 1, z, z, z, z, z, z, z, 1, 1, z, z, z, z, z, z, z, z) == -1


def test_grasp_chain_module_is_importable():
    from grasptrajopt_amd.grasp_chain import GraspChain
    assert callable(GraspChain.plan_objects) and callable(GraspChain.bind_scene)


def test_choice_is_first_of_lexsort_with_ties_and_nans():
    rng = np.random.default_rng(0)
    for trial in range(400):
        n = int(rng.integers(1, 40))
        cost = rng.integers(0, 3, n).astype(np.float64) * 0.5  # many ties
        dist = rng.integers(0, 4, n).astype(np.float64)
        cost[rng.random(n) < 0.2] = np.nan
        dist[rng.random(n) < 0.2] = np.nan
        if trial % 7 == 0:
            cost[:] = np.nan
        if trial % 11 == 0:
            cost[rng.random(n) < 0.3] = -0.0
        assert ref.choose(cost, dist) == int(np.lexsort((dist, cost))[0]), (cost, dist)


def test_candidates_are_interpolate_waypoints_bit_for_bit():
    from grasptrajopt_amd import utils
    rng = np.random.default_rng(1)
    for T in (4, 50, 96):
        ndof, n = 9, 6
        qc, qs = rng.uniform(-2, 2, ndof), rng.uniform(-3, 3, (n, ndof))
        param = np.array([7, 8])
        for f32 in (False, True):
            got = ref.candidates(qc, qs, T, param, f32)
            src = qs.astype(np.float32).astype(np.float64) if f32 else qs
            for i in range(n):
                want = utils.interpolate_waypoints(np.stack([qc, src[i]]), T, ndof)
                want[:, param] = qc[param]
                assert got[i].tobytes() == np.ascontiguousarray(want.T).tobytes()


def test_compaction_and_the_branch_without_a_solution():
    rng = np.random.default_rng(2)
    n_max, ndof, T = 7, 9, 50
    goals, qs, qc = rng.standard_normal((n_max, 16)), rng.uniform(-1, 1, (n_max, ndof)), rng.uniform(-1, 1, ndof)
    accept = np.array([0, 1, 1, 0, 1, 1, 1], dtype=np.uint8)
    score = lambda plans: np.abs(plans[:, 0, -1])
    r = ref.seed_goalsets(qc, goals, 5, qs, accept, T, -10, [7, 8], True, False, score)  # rows 5 and 6 do not count
    assert r["n_accepted"] == r["n_goals_out"] == 3 and np.array_equal(r["goals_out"], goals[[1, 2, 4]])
    assert r["seed_index"] == int(np.argmin(np.abs(r["plans"][:, 0, -1]))) and np.array_equal(r["Q0"], r["plans"][r["seed_index"]])
    assert np.array_equal(ref.accepted_rows(99, n_max, accept), [1, 2, 4, 5, 6]) and np.array_equal(ref.accepted_rows(-3, n_max, accept), [])
    assert np.array_equal(ref.accepted_rows(3, n_max, None), [0, 1, 2])
    r = ref.seed_goalsets(qc, goals, 4, qs, np.zeros(n_max, np.uint8), T, -10, [7, 8], True, False, score)
    assert (r["n_accepted"], r["n_goals_out"], r["seed_index"]) == (0, 4, -1)
    assert np.array_equal(r["goals_out"], goals[:4]) and np.array_equal(r["Q0"], np.tile(qc[:, None], (1, T)))


def test_seed_without_interpolation_is_the_planners_construction():
    rng = np.random.default_rng(3)
    ndof, T, off = 9, 50, -10
    qc, qs = rng.uniform(-1, 1, ndof), rng.uniform(-2, 2, (3, ndof))
    plans = ref.candidates(qc, qs, T, [7, 8])
    Q0 = np.diag(qc) @ np.ones((ndof, T))  # grasptrajopt_amd/gto_planner.py:110-113
    for i in range(T + off, T):
        Q0[:, i] = plans[1][:, T - 1]
    assert ref.seed_from(qc, plans[1], False, T, off).tobytes() == Q0.tobytes()
    assert ref.seed_from(qc, plans[1], True, T, off).tobytes() == plans[1].tobytes()


def test_report_rule_is_false_on_nan():
    RT = np.tile(np.eye(4), (3, 1, 1))
    Tee = RT.copy()
    Tee[1, 0, 3] = np.nan
    ep, er, acc = ref.report(Tee, RT, np.array([0.0, 0.0, np.nan]), 0.01, 5.0, 5.0)
    assert acc.tolist() == [True, False, False] and ep[0] == 0.0 and er[0] == 0.0
