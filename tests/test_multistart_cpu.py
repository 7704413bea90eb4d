"""CPU: the multi-seed entry points exist (header, exports, ABI still 1012), refuse a null handle and an n_seeds outside
[1, 16] before any device work, and the numpy restatement the GPU tests compare against (tests/multistart_ref.py) is itself
pinned to np.lexsort and to the class table of include/gto_solver.h."""
import os
import re

import numpy as np
import pytest

import multistart_ref as mref
from conftest import ROOT

NEW = ("gto_seed_goalsets_multi_device", "gto_plan_report_device", "gto_select_plans_device")
NAN = float("nan")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


def test_symbols_are_exported_declared_and_abi_is_still_1012(capi):
    hdr = open(os.path.join(ROOT, "include", "gto_solver.h")).read()
    assert int(re.search(r"#define GTO_ABI_VERSION (\d+)", hdr).group(1)) == 1012 == capi.ABI_VERSION
    assert int(re.search(r"#define GTO_MAX_SEEDS (\d+)", hdr).group(1)) == 16
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = capi.load_library()
    assert lib.gto_version() == 1012
    for sym in NEW:
        assert re.search(rf"\bint {sym}\s*\(", code), sym
        assert sym in capi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    for m in ("seed_goalsets_multi_device", "plan_report_device", "select_plans_device"):
        assert callable(getattr(capi.SolverHandle, m))


def seeds_multi(lib, n_seeds):
    z = None
    return lib.gto_seed_goalsets_multi_device(None, 1, 1, n_seeds, z, z, z, z, z, z, z, 1, 1, z, z, z, z, z, z, z, z, z)


def select(lib, n_seeds):
    z = None
    return lib.gto_select_plans_device(None, 1, n_seeds, z, z, z, z, z, 0.01, 5.0, 5, z, z, z, z, z, z, z)


def test_null_handle_is_invalid_arg(capi):
    lib = capi.load_library()
    z = None
    assert seeds_multi(lib, 1) == -1 and seeds_multi(lib, 16) == -1
    assert lib.gto_plan_report_device(None, 1, 1, z, z, z, z, z, z, z, z, z) == -1
    assert select(lib, 1) == -1 and select(lib, 16) == -1


def test_n_seeds_0_and_17_are_refused_before_any_device_work(capi):
    """GTO_ERR_UNSUPPORTED (-4) without so much as a handle: the number is looked at first."""
    lib = capi.load_library()
    for n_seeds in (0, 17, -1):
        assert seeds_multi(lib, n_seeds) == -4, n_seeds
        assert b"n_seeds must be in [1, 16]" in lib.gto_last_error(None)
        assert select(lib, n_seeds) == -4, n_seeds


def test_plan_objects_takes_n_seeds_and_max_points():
    import inspect
    from grasptrajopt_amd.grasp_chain import GraspChain
    p = inspect.signature(GraspChain.plan_objects).parameters
    assert p["n_seeds"].default == 1 and p["max_points"].default == 5


def test_ranked_choice_is_the_head_of_lexsort_with_ties_and_nans():
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
        for k in (1, 2, 3, 16, 40):
            assert mref.choose_ranked(cost, dist, k) == np.lexsort((dist, cost))[:k].tolist(), (cost, dist, k)


def test_slots_behind_the_accepted_rows_and_without_one():
    rng = np.random.default_rng(2)
    n_max, ndof, T = 7, 9, 50
    goals, qs, qc = rng.standard_normal((n_max, 16)), rng.uniform(-1, 1, (n_max, ndof)), rng.uniform(-1, 1, ndof)
    accept = np.array([0, 1, 1, 0, 1, 1, 1], dtype=np.uint8)
    score = lambda plans: np.abs(plans[:, 0, -1])
    r = mref.seed_slots(qc, goals, 5, qs, accept, T, -10, [7, 8], True, False, score, 4)  # rows 5 and 6 do not count
    order = np.argsort(np.abs(r["plans"][:, 0, -1]), kind="stable")
    assert r["rows"].tolist() == [1, 2, 4] and r["seed_index"].tolist() == order.tolist() + [-1]
    for s in range(3):
        assert np.array_equal(r["Q0"][s], r["plans"][order[s]])
    assert np.array_equal(r["Q0"][3], r["Q0"][0])
    r = mref.seed_slots(qc, goals, 4, qs, np.zeros(n_max, np.uint8), T, -10, [7, 8], True, False, score, 3)
    assert r["seed_index"].tolist() == [-1, -1, -1] and np.array_equal(r["Q0"], np.tile(qc[None, :, None], (3, 1, T)))


TABLE, table = mref.CLASS_TABLE, mref.class_table


def test_class_rule_and_selection_order():
    args, want = table(range(len(TABLE)))
    best, cls, all_cls = mref.select(*args, 0.01, 5.0, 5)
    assert all_cls == want and set(want) == {0, 1, 2, 3, 4}
    assert (best, cls) == (0, 0)                                   # the tie on (class, cost) goes to the lower slot
    assert mref.select(*table([9, 0])[0], 0.01, 5.0, 5)[:2] == (0, 0)
    assert mref.select(*table([1, 2, 3, 5])[0], 0.01, 5.0, 5)[:2] == (0, 1)   # class before cost: 2.0 in class 1 beats 1.0 in class 2
    assert mref.select(*table([2, 1])[0], 0.01, 5.0, 5)[:2] == (1, 1)         # the lower cost within a class
    assert mref.select(*table([7, 8, 6])[0], 0.01, 5.0, 5)[:2] == (2, 4)      # class 4: 0.1, then inf, then the NaN
    assert mref.select(*table([7, 8])[0], 0.01, 5.0, 5)[:2] == (1, 4)
    assert mref.select(*table([7, 7])[0], 0.01, 5.0, 5)[:2] == (0, 4)
    assert mref.select(*table([4, 3])[0], 0.01, 5.0, 5)[:2] == (1, 2)
    # without counts every slot is free
    a = table([3, 4, 0])[0]
    assert mref.select(*a[:4], None, 0.01, 5.0, 5) == (0, 0, [0, 0, 0])
    # the order is the sort by (class, cost with a NaN last, slot)
    rng = np.random.default_rng(5)
    for _ in range(200):
        rows = rng.integers(0, len(TABLE), int(rng.integers(1, 17)))
        a, want = table(rows)
        key = sorted(range(len(rows)), key=lambda s: (want[s], np.isnan(a[1][s]), 0.0 if np.isnan(a[1][s]) else a[1][s], s))
        assert mref.select(*a, 0.01, 5.0, 5)[0] == key[0]
