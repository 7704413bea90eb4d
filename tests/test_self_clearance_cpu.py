"""CPU: the self-clearance check's symbols, host-side validation, link-pair rule and numpy restatement, and the proof that
the inputs of tests/test_gpu_self_clearance.py exercise something (the oracle's kinematics on the same columns and masks)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import self_clearance_ref as R
import small_robots as sr
from conftest import ROOT

NAMES = {"gto_set_self_pairs": 2, "gto_self_clearance": 7, "gto_self_clearance_device": 8}  # name -> arguments


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


# ---------------------------------------------------------------------------------------------- symbols
def test_symbols_are_declared_exported_and_bound(capi):
    hdr = open(os.path.join(ROOT, "include", "gto_solver.h")).read()
    assert int(re.search(r"#define GTO_ABI_VERSION (\d+)", hdr).group(1)) == 1012 == capi.ABI_VERSION  # additions keep it
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = capi.load_library()
    assert lib.gto_version() == 1012
    for name, n_args in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in include/gto_solver.h"
        assert len(m.group(1).split(",")) == n_args, name
        assert name in capi.EXPORTED_SYMBOLS and len(capi.PROTOTYPES[name][1]) == n_args, name
        assert hasattr(lib, name), name


# ---------------------------------------------------------------------------------------------- validation without a device
def test_arguments_are_refused_before_any_device_call(capi):
    """Through the library itself: the argument checks come before the handle is touched, so a null handle shows them."""
    lib = capi.load_library()

    def last():
        return lib.gto_last_error(None).decode()
    d2, pair, paths = (C.c_double * 4)(), (C.c_int32 * 8)(), (C.c_double * 64)()
    for B, Tp, cutoff, why in [(1, 0, 1.0, "Tp >= 1"), (-1, 2, 1.0, "B >= 0"), (1, 2, float("nan"), "cutoff"), (1, 2, 0.0, "cutoff"),
                               (1, 2, -0.5, "cutoff")]:
        assert lib.gto_self_clearance(None, B, Tp, paths, cutoff, d2, pair) == -1 and why in last(), (B, Tp, cutoff)
        assert lib.gto_self_clearance_device(None, B, Tp, None, cutoff, None, None, None) == -1 and why in last(), (B, Tp, cutoff)
    assert lib.gto_set_self_pairs(None, None) == -1  # (a null handle)


def test_the_mask_rules_under_sanitizers(tmp_path):
    """check_self_pairs / check_self_clearance_args / all_distinct_pairs of csrc/gto_selfpairs.h in a stand-alone program built
    with AddressSanitizer and UBSan, on arrays of exactly n_links words, 1 and 32 links included."""
    exe = tmp_path / "self_pairs"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "grasptrajopt_amd", "csrc"),
                           os.path.join(ROOT, "tests", "self_pairs_main.cpp"), "-o", str(exe)])

    def run(*args):
        res = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout.strip()
    ok = "rc=0 why="
    full32 = [0xFFFFFFFF & ~(1 << a) for a in range(32)]
    assert run("mask", 1, 0) == ok and run("mask", 3, 0b110, 0b101, 0b011) == ok and run("mask", 32, *full32) == ok
    assert run("mask", 3, 0, 0, 0) == ok
    assert run("mask", 3, 0b100, 0, 0) == "rc=-1 why=gto_set_self_pairs: the mask is not symmetric"
    assert run("mask", 3, 0b001, 0, 0) == "rc=-1 why=gto_set_self_pairs: a link is paired with itself"
    assert run("mask", 3, 0b1000, 0, 0) == "rc=-1 why=gto_set_self_pairs: a bit at or above n_links is set"
    assert run("mask", 1, 1) == "rc=-1 why=gto_set_self_pairs: a link is paired with itself"
    bad32 = list(full32)
    bad32[31] &= ~1  # (31, 0) off, (0, 31) on
    assert run("mask", 32, *bad32) == "rc=-1 why=gto_set_self_pairs: the mask is not symmetric"
    assert run("args", 0, 1, "inf") == ok and run("args", 5, 1, 0.01) == ok
    assert run("args", 1, 0, 1.0).startswith("rc=-1") and run("args", -1, 1, 1.0).startswith("rc=-1")
    for c in ("nan", "0", "-1"):
        assert run("args", 1, 1, c) == "rc=-1 why=gto_self_clearance: the cutoff must be > 0 (+inf: none)"
    assert run("default", 3).split()[:4] == ["6", "5", "3", "0"]
    assert run("default", 32).split() == [str(w) for w in full32]


def test_mask_words(capi):
    M = np.zeros((12, 12), dtype=bool)
    M[0, 11] = M[11, 0] = M[2, 5] = M[5, 2] = True
    rows = capi.self_pair_rows(M, 12)
    assert rows.dtype == np.int32 and rows.tolist() == [1 << 11, 0, 1 << 5, 0, 0, 1 << 2, 0, 0, 0, 0, 0, 1]
    full = ~np.eye(32, dtype=bool)
    assert capi.self_pair_rows(full, 32).view(np.uint32).tolist() == [0xFFFFFFFF & ~(1 << a) for a in range(32)]
    with pytest.raises(ValueError, match="must be"):
        capi.self_pair_rows(M, 11)


# ---------------------------------------------------------------------------------------------- which pairs count
def robots():
    from grasptrajopt_amd.robot_desc import load_builtin
    out = [(name, load_builtin(name), R.config(name)["default_pose"]) for name in R.ROBOTS]
    return out + [(k, sr.Robot(k).desc, None) for k in sr.KINDS]


def test_self_pairs_rule():
    for name, d, q_ref in robots():
        for M in (d.self_pairs(), d.self_pairs(q_ref=q_ref) if q_ref is not None else d.self_pairs(q_ref=np.zeros(d.ndof))):
            assert M.shape == (d.n_links, d.n_links) and M.dtype == bool, name
            assert np.array_equal(M, M.T) and not M.diagonal().any(), name
    by = {name: (d, q) for name, d, q in robots()}
    d, q = by["panda"]
    ix = d.link_names.index
    plain, rest = d.self_pairs(), d.self_pairs(q_ref=q)
    assert plain.sum() // 2 == 48 and rest.sum() // 2 == 47
    for a in range(7):  # neighbours along the arm
        assert not plain[ix(f"panda_link{a}"), ix(f"panda_link{a + 1}")]
    for a, b in [("panda_hand", "panda_leftfinger"), ("panda_hand", "panda_rightfinger"), ("panda_link7", "panda_hand"),
                 ("panda_link6", "panda_hand")]:
        assert not plain[ix(a), ix(b)], (a, b)
    assert plain[ix("panda_link0"), ix("panda_hand")] and rest[ix("panda_link0"), ix("panda_hand")]
    assert rest[ix("panda_link5"), ix("panda_link7")]  # 3.5 cm at rest: stays
    lf, rf = ix("panda_leftfinger"), ix("panda_rightfinger")
    assert plain[lf, rf] and not rest[lf, rf]  # 1 mm apart at rest: off only with q_ref
    assert set(zip(*np.nonzero(np.triu(plain & ~rest)))) == {(lf, rf)}
    ign = d.self_pairs(q_ref=q, ignore=[("panda_hand", "panda_link0"), ("panda_link5", "panda_link7")])
    assert ign.sum() // 2 == 45 and not ign[ix("panda_link0"), ix("panda_hand")] and not ign[ix("panda_link7"), ix("panda_link5")]
    d, q = by["fetch"]
    plain, rest = d.self_pairs(), d.self_pairs(q_ref=q)
    assert plain.sum() // 2 == 33 and rest.sum() // 2 == 32
    fa, fb = d.link_names.index("r_gripper_finger_link"), d.link_names.index("l_gripper_finger_link")
    assert set(zip(*np.nonzero(np.triu(plain & ~rest)))) == {(min(fa, fb), max(fa, fb))}
    # robots whose links are all neighbours: nothing to compare
    for k in ("chain_1", "one_point", "static_links_only", "root_joint"):
        assert not by[k][0].self_pairs().any(), k
    assert by["chain_3"][0].self_pairs().sum() // 2 == 3  # (0, 2), (0, 3), (1, 3) of four links in a row


def test_point_spacing():
    from grasptrajopt_amd.robot_desc import load_builtin
    assert load_builtin("panda").point_spacing() == pytest.approx(0.0170, abs=1e-4)
    assert load_builtin("fetch").point_spacing() == pytest.approx(0.0148, abs=1e-4)
    assert sr.Robot("one_point").desc.point_spacing() == 0.0  # no link with two points


def test_world_points_agree_with_the_oracle(oracle_mod):
    from grasptrajopt_amd.robot_desc import load_builtin
    for name in R.ROBOTS:
        d, cfg = load_builtin(name), R.config(name)
        orc = oracle_mod.Oracle(d, cfg["link_ee"], cfg["link_gripper"], oracle_mod.reference_opts())
        q = R.robot_columns(name, d)[:3]
        X = orc.eval_points(0, q, [0.0, 0.0, 0.0], want_field=False)[0]
        for i in range(3):
            assert np.abs(d.world_points(q[i]) - X[i]).max() < 1e-12, name


# ---------------------------------------------------------------------------------------------- the restatement
def test_reference_on_hand_made_points():
    link = np.array([0, 0, 1, 1, 2])
    X = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 0.5, 0], [4.0, 0, 0], [1.0, 0, -0.5]])
    full = ~np.eye(3, dtype=bool)
    # links 0 and 1 are 0.5 apart, and so are links 0 and 2: the tie goes to (0, 1); links 1 and 2 are sqrt(0.5) apart
    assert R.reference(X, link, full) == (0.25, (0, 1))
    assert R.reference(X, link, None) == (0.25, (0, 1))
    only = lambda a, b: R.single_pair_mask(type("D", (), {"link_names": ["a", "b", "c"], "n_links": 3}), ("abc"[a], "abc"[b]))  # noqa: E731
    assert R.reference(X, link, only(0, 2)) == (0.25, (0, 2))
    assert R.reference(X, link, only(1, 2)) == (0.5, (1, 2))
    assert R.reference(X, link, full, cutoff=0.4) == (0.4 * 0.4, (-1, -1))  # below the minimum
    assert R.reference(X, link, full, cutoff=0.5) == (0.25, (-1, -1))        # at it: "closer than" is strict
    assert R.reference(X, link, full, cutoff=0.6) == (0.25, (0, 1))          # above it
    assert R.reference(X, link, np.zeros((3, 3), dtype=bool)) == (np.inf, (-1, -1))
    assert R.reference(X, link, np.zeros((3, 3), dtype=bool), cutoff=2.0) == (4.0, (-1, -1))
    bad = X.copy()
    bad[3, 1] = np.nan
    d2, pair = R.reference(bad, link, full)
    assert np.isnan(d2) and pair == (-1, -1)
    # the expression: (dx*dx + dy*dy) + dz*dz, one rounding each
    a, b = np.array([[0.1, 0.2, 0.3]]), np.array([[0.7, -0.4, 0.9]])
    dx, dy, dz = a[0] - b[0]
    assert R.pair_d2(a, b) == (dx * dx + dy * dy) + dz * dz
    d2c, pc = R.apply_cutoff(np.array([0.25, 0.01]), np.array([[0, 1], [1, 2]], dtype=np.int32), 0.3)
    assert d2c.tolist() == [0.3 * 0.3, 0.01] and pc.tolist() == [[-1, -1], [1, 2]]


def test_summary_per_path(capi):
    d2 = np.array([[0.04, 0.01, 0.09], [0.04, np.nan, 0.0001], [0.04, 0.04, 0.04]])
    pair = np.arange(18, dtype=np.int32).reshape(3, 3, 2)
    got = capi.self_check_summary(d2, pair, 0.15)
    assert got["self_d2"][0] == 0.01 and np.isnan(got["self_d2"][1]) and got["self_d2"][2] == 0.04
    assert got["self_pair"].tolist() == [[2, 3], [8, 9], [12, 13]]
    assert got["self_clear"].tolist() == [False, False, True]
    with pytest.raises(TypeError, match="unexpected key"):
        capi.self_check_request(sr.Robot("chain_3").desc, dict(clearence=0.1))


# ---------------------------------------------------------------------------------------------- the GPU tests' inputs
def test_the_gpu_cases_exercise_something(oracle_mod):
    """On the oracle's world points of the columns and masks tests/test_gpu_self_clearance.py runs: at least 3 columns
    below the default clearance, at least 3 above twice it, at least 6 distinct closest link pairs -- under the masks a
    planner would use (not the never-set "all pairs", under which every column has two neighbours touching)."""
    from grasptrajopt_amd.robot_desc import load_builtin
    below = above = 0
    pairs = set()
    for name in R.ROBOTS:
        d, cfg = load_builtin(name), R.config(name)
        orc = oracle_mod.Oracle(d, cfg["link_ee"], cfg["link_gripper"], oracle_mod.reference_opts())
        X = orc.eval_points(0, R.robot_columns(name, d), [0.0, 0.0, 0.0], want_field=False)[0]
        clearance = d.point_spacing()
        seen = {}
        for mname, M in R.masks(name, d).items():
            if mname in ("unset", "empty"):
                continue
            res = [R.reference(X[i], d.point_link, M) for i in range(len(X))]
            seen[mname] = {p for _, p in res}
            pairs |= {(name, p) for _, p in res}
            if mname == "default":
                dist = np.sqrt([r[0] for r in res])
                below += int((dist < clearance).sum())
                above += int((dist > 2 * clearance).sum())
        assert len(seen["default"]) >= 3 and len(seen["far"]) >= 3, name
        print(name, {k: len(v) for k, v in seen.items()})
    print("below", below, "above", above, "distinct pairs", len(pairs))
    assert below >= 3 and above >= 3 and len(pairs) >= 6
