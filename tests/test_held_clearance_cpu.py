"""CPU: the held-clearance check's symbols, host-side validation, link rule, numpy restatement and summary, and the proof that
the inputs of tests/test_gpu_held_clearance.py exercise something (the oracle's kinematics on the same columns)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import held_clearance_ref as H
import self_clearance_ref as SR
import small_robots as sr
from conftest import ROOT

NAMES = {"gto_held_clearance": 18, "gto_held_clearance_device": 19}  # name -> arguments


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


def test_the_build_refuses_scratch_for_the_kernel(capi):
    """The kernel is on the list of the build's no-scratch check, and the report of the build that made the library shows
    it without scratch."""
    import __graft_entry__ as g
    assert "k_held_clearance" in g.KERNEL_NO_SCRATCH
    report = os.path.join(g.CSRC, "kernel_resources.txt")
    rows = [line for line in open(report) if "k_held_clearance" in line]
    assert len(rows) == 1 and "ScratchSize=0 " in rows[0], rows


# ---------------------------------------------------------------------------------------------- validation without a device
def test_arguments_are_refused_before_any_device_call(capi):
    """Through the library itself: the argument checks come before the handle is touched, so a null handle shows them."""
    lib = capi.load_library()

    def last():
        return lib.gto_last_error(None).decode()
    d = (C.c_double * 64)()
    n = (C.c_int32 * 4)()
    base = (C.c_double * 3)()
    inf = float("inf")

    def host(B=1, Tp=2, paths=d, attach=None, ld=0, col=0, pts=d, P=4, n_held=n, base_pos=base, mask=1, cutoff=inf, d2=d):
        return lib.gto_held_clearance(None, B, Tp, paths, attach, ld, col, pts, P, n_held, None, base_pos, 0, mask, cutoff, d2, None, None)

    def device(B=1, Tp=2, paths=1, attach=None, ld=0, col=0, pts=1, P=4, n_held=1, base_pos=base, mask=1, cutoff=inf, d2=1):
        return lib.gto_held_clearance_device(None, B, Tp, paths, attach, ld, col, pts, P, n_held, None, base_pos, 0, mask, cutoff, d2,
                                             None, None, None)
    for call, arr in ((host, d), (device, 1)):
        for kw, why in [(dict(Tp=0), "Tp >= 1"), (dict(B=-1), "B >= 0"), (dict(P=0), "P_max >= 1"),
                        (dict(cutoff=float("nan")), "cutoff"), (dict(cutoff=0.0), "cutoff"), (dict(cutoff=-0.5), "cutoff"),
                        (dict(attach=arr, ld=3, col=3), "attach_col"), (dict(attach=arr, ld=3, col=-1), "attach_col"),
                        (dict(base_pos=None), "null base"), (dict(paths=None), "null paths"), (dict(pts=None), "null paths"),
                        (dict(n_held=None), "null paths"), (dict(d2=None), "null paths")]:
            assert call(**kw) == -1 and why in last(), (call.__name__, kw, last())
        assert call(B=70000) == -4 and "65535" in last()
        assert call() == -1  # (all in order: the null handle is what is left)
        assert call(B=0, paths=None, pts=None, n_held=None, d2=None) == -1  # (even an empty batch needs a handle)


def test_the_argument_rules_under_sanitizers(tmp_path):
    """check_held_clearance_args of csrc/gto_heldargs.h in a stand-alone program built with AddressSanitizer and UBSan: the
    link mask against the handle's number of links, 1 and 32 links included."""
    exe = tmp_path / "held_args"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "grasptrajopt_amd", "csrc"),
                           os.path.join(ROOT, "tests", "held_args_main.cpp"), "-o", str(exe)])

    def run(n_links, mask, B=1, Tp=2, P=4, attach=0, ld=0, col=0, cutoff="inf", arrays=1):
        res = subprocess.run([str(exe)] + [str(a) for a in (n_links, B, Tp, P, attach, ld, col, mask, cutoff, arrays)],
                             capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout.strip()
    ok = "rc=0 empty=0 why="
    high = "rc=-1 empty=0 why=gto_held_clearance: a link_mask bit at or above n_links is set"
    assert run(12, 0) == ok and run(12, 0b111111) == ok and run(12, (1 << 12) - 1) == ok
    assert run(12, 1 << 12) == high and run(12, 1 << 31) == high and run(1, 2) == high
    assert run(1, 1) == ok and run(32, 0xFFFFFFFF) == ok and run(32, 1 << 31) == ok
    assert run(12, 1 << 12, B=0) == high.replace("empty=0", "empty=1")  # the mask is judged for an empty batch too
    assert run(12, 1, B=0, arrays=0) == "rc=0 empty=1 why="
    assert run(12, 1, arrays=0).startswith("rc=-1") and run(12, 1, cutoff="nan").startswith("rc=-1")
    assert run(12, 1, attach=1, ld=5, col=4) == ok and run(12, 1, attach=1, ld=5, col=5).startswith("rc=-1")
    assert run(12, 1, attach=0, ld=0, col=7) == ok  # (attach NULL: the column is not read)
    assert run(12, 1, B=65535, P=65535) == ok and run(12, 1, B=65536).startswith("rc=-4") and run(12, 1, P=65536).startswith("rc=-4")


def test_mask_word(capi):
    m = np.zeros(12, dtype=bool)
    m[[0, 5, 11]] = True
    assert capi.held_link_mask(m, 12) == (1 | 1 << 5 | 1 << 11)
    assert capi.held_link_mask(np.ones(32, dtype=bool), 32) == -1  # the 32 bits of an unsigned word, as int32
    assert capi.held_link_mask(np.zeros(3, dtype=bool), 3) == 0
    with pytest.raises(ValueError, match="must be"):
        capi.held_link_mask(m, 11)


# ---------------------------------------------------------------------------------------------- which links count
def test_held_links_rule():
    from grasptrajopt_amd.robot_desc import load_builtin
    for name in H.ROBOTS:
        d, spec = load_builtin(name), H.HELD[name]
        assert SR.config(name)["link_ee"] == spec["link_ee"]
        m = d.held_links(spec["link_ee"])
        assert m.shape == (d.n_links,) and m.dtype == bool
        assert [n for n, on in zip(d.link_names, m) if on] == spec["expect"], name
        less = d.held_links(spec["link_ee"], ignore=spec["expect"][:2])
        assert [n for n, on in zip(d.link_names, less) if on] == spec["expect"][2:], name
    # four links in a row, the object on the last: the two links with two joints or more in between
    d = sr.Robot("chain_3").desc
    assert d.held_links("f3").tolist() == [True, True, False, False] and d.held_links("f0").tolist() == [False, False, True, True]
    for k in ("chain_1", "one_point", "static_links_only", "root_joint"):
        rb = sr.Robot(k)
        assert not rb.desc.held_links(rb.ee).any(), k
    with pytest.raises(KeyError):
        d.held_links("no_such_frame")


def test_request_and_summary(capi):
    from grasptrajopt_amd.robot_desc import load_builtin
    d = load_builtin("panda")
    c, cut, links = capi.held_clearance_request(d, "panda_hand", {})
    assert c == d.point_spacing() and cut == 2 * c and np.array_equal(links, d.held_links("panda_hand"))
    c, cut, links = capi.held_clearance_request(d, "panda_hand", dict(clearance=0.03, ignore=["panda_link0"]))
    assert (c, cut) == (0.03, 0.06) and not links[0] and links[1:6].all() and not links[6:].any()
    every = np.ones(d.n_links, dtype=bool)
    c, cut, links = capi.held_clearance_request(d, "panda_hand", dict(cutoff=np.inf, links=every, ignore=["panda_hand"]))
    assert cut == np.inf and links.sum() == d.n_links - 1 and every.all()  # (the caller's array is not written)
    with pytest.raises(TypeError, match="unexpected key"):
        capi.held_clearance_request(d, "panda_hand", dict(clearence=0.1))
    with pytest.raises(ValueError, match="> 0"):
        capi.held_clearance_request(d, "panda_hand", dict(cutoff=0.0))
    with pytest.raises(ValueError, match="must be"):
        capi.held_clearance_request(d, "panda_hand", dict(links=np.ones(3, dtype=bool)))
    d2 = np.array([[0.04, 0.01, 0.09], [0.04, np.nan, 0.0001], [0.04, 0.04, 0.04]])
    link = np.arange(9, dtype=np.int32).reshape(3, 3)
    point = 100 + link
    got = capi.held_clearance_summary(d2, link, point, 0.15, "x_")
    assert sorted(got) == ["x_clear", "x_col", "x_d2", "x_link", "x_point"]
    assert got["x_d2"][0] == 0.01 and np.isnan(got["x_d2"][1]) and got["x_d2"][2] == 0.04
    assert got["x_col"].tolist() == [1, 1, 0] and got["x_link"].tolist() == [1, 4, 6] and got["x_point"].tolist() == [101, 104, 106]
    assert got["x_clear"].tolist() == [False, False, True]
    assert sorted(capi.held_clearance_summary(d2, link, point, 0.15)) == ["held_self_clear", "held_self_col", "held_self_d2",
                                                                        "held_self_link", "held_self_point"]


# ---------------------------------------------------------------------------------------------- the restatement
def test_reference_on_hand_made_points():
    plink = np.array([0, 0, 1, 1, 2])
    X = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 1.0, 0], [4.0, 0, 0], [1.0, 0.5, -0.5]])
    Y = np.array([[1.0, 0.5, 0.0], [0.5, 0.0, 0.0], [1.0, 0.5, 0.0], [9.0, 9.0, 9.0]])
    every = np.ones(3, dtype=bool)
    # held points 0 and 2 are one point: 0.5 from link 0 (its point 1), from link 1 and from link 2; held point 1 is 0.5 from
    # link 0 as well: the tie between links goes to link 0, the tie between held points to point 0
    assert H.reference(X, plink, every, Y) == (0.25, 0, 0)
    assert H.reference(X, plink, [False, True, True], Y) == (0.25, 1, 0)
    assert H.reference(X, plink, [False, False, True], Y) == (0.25, 2, 0)
    assert H.reference(X, plink, every, Y[1:]) == (0.25, 0, 0)      # held points 1 and 2 of before: both 0.5 from link 0
    assert H.reference(X, plink, every, Y[2:]) == (0.25, 0, 0)
    assert H.reference(X, plink, every, Y, cutoff=0.4) == (0.4 * 0.4, -1, -1)  # below the minimum
    assert H.reference(X, plink, every, Y, cutoff=0.5) == (0.25, -1, -1)        # at it: "closer than" is strict
    assert H.reference(X, plink, every, Y, cutoff=0.6) == (0.25, 0, 0)          # above it
    assert H.reference(X, plink, np.zeros(3, dtype=bool), Y) == (np.inf, -1, -1)          # the empty mask
    assert H.reference(X, plink, np.zeros(3, dtype=bool), Y, cutoff=2.0) == (4.0, -1, -1)
    assert H.reference(X, plink, every, Y[:0]) == (np.inf, -1, -1)                        # n_held = 0
    assert H.reference(X, plink, [False, False, False, True], Y) == (np.inf, -1, -1)      # an enabled link without points
    nan = Y.copy()
    nan[0, 1] = np.nan  # a NaN held point is skipped: point 1 is next, and nobody else's index moves
    assert H.reference(X, plink, every, nan) == (0.25, 0, 1)
    assert H.reference(X, plink, [False, True, False], nan) == (0.25, 1, 2)
    bad = X.copy()
    bad[3, 1] = np.inf
    d2, link, point = H.reference(bad, plink, every, Y)
    assert np.isnan(d2) and (link, point) == (-1, -1)
    # the expression: (dx*dx + dy*dy) + dz*dz of d = Y - X, one rounding each
    a, b = np.array([[0.1, 0.2, 0.3]]), np.array([[0.7, -0.4, 0.9]])
    dx, dy, dz = b[0] - a[0]
    assert H.reference(a, np.array([0]), [True], b)[0] == (dx * dx + dy * dy) + dz * dz
    d2c, lc, pc = H.apply_cutoff(np.array([0.25, 0.01]), np.array([3, 4], dtype=np.int32), np.array([7, 8], dtype=np.int32), 0.3)
    assert d2c.tolist() == [0.3 * 0.3, 0.01] and lc.tolist() == [-1, 4] and pc.tolist() == [-1, 8]


def test_carried_points_are_the_held_check_formulas_without_the_base():
    import held_ref as HR
    rng = np.random.default_rng(5)
    E = np.tile(np.eye(4), (3, 1, 1))
    for t in range(3):
        E[t, :3, :3], E[t, :3, 3] = HR._rotation(rng), rng.uniform(-0.5, 0.5, 3)
    x, base = rng.uniform(-0.3, 0.3, (9, 3)), np.array([0.4, -0.3, 0.2])
    Y = H.carried(E, E[0], base, x)
    assert Y.shape == (3, 9, 3) and np.abs(Y[0] - (x - base)).max() < 1e-15  # at the grasp: where the points are, seen from the base
    assert np.abs(Y + base - HR.held_world(E, E[0], base, x)).max() < 1e-15
    assert np.array_equal(Y, HR.carry(HR.attach(x, base, E[0]), E, np.zeros(3)))
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = HR._rotation(rng), [0.1, 0.2, 0.3]
    assert np.array_equal(H.carried(E, E[0], base, x, pose), H.carried(E, E[0], base, HR.place(x, pose)))


def test_the_box():
    for name in H.ROBOTS:
        pts = H.box(name)
        centre = np.zeros(3)
        centre[H.HELD[name]["axis"]] = H.HELD[name]["offset"]
        u = (pts - centre) / np.array(H.BOX_SIZE)
        assert pts.shape == (H.N_BOX, 3) and np.abs(u).max() <= 0.5 + 1e-12
        assert (np.isclose(np.abs(u), 0.5).sum(axis=1) >= 1).all()  # every sample lies on a face
    assert np.abs((H.box("panda") - [0, 0, 0.10]) - (H.box("fetch") - [0.17, 0, 0])).max() < 1e-15  # one box, two centres


# ---------------------------------------------------------------------------------------------- the GPU tests' inputs
def test_the_gpu_cases_exercise_something(oracle_mod):
    """On the oracle's world points and link_ee frames of the 20 columns tests/test_gpu_held_clearance.py runs, under the
    planners' default links: per robot at least MUST_EXERCISE columns below the default clearance, beyond the default
    cutoff (twice it), and distinct closest links among the near ones."""
    from grasptrajopt_amd.robot_desc import load_builtin
    for name in H.ROBOTS:
        d, cfg, spec = load_builtin(name), SR.config(name), H.HELD[name]
        orc = oracle_mod.Oracle(d, cfg["link_ee"], cfg["link_gripper"], oracle_mod.reference_opts())
        q = H.robot_columns(name, d)
        assert q.shape == (20, d.ndof)
        X = orc.eval_points(0, q, [0.0, 0.0, 0.0], want_field=False)[0]
        fe = d.frame_index(spec["link_ee"])
        E_t, E_a = orc.eval_fk(q)[:, fe], orc.eval_fk(H.grasp_pose(name)[None])[0, fe]
        Y = H.carried(E_t, E_a, H.BASE, H.held_world(E_a, H.BASE, H.box(name)))
        clearance = d.point_spacing()
        res = [H.reference(X[i], d.point_link, d.held_links(spec["link_ee"]), Y[i]) for i in range(len(q))]
        dist = np.sqrt([r[0] for r in res])
        below, beyond = int((dist < clearance).sum()), int((dist > 2 * clearance).sum())
        near_links = {r[1] for r, dd in zip(res, dist) if dd < clearance}
        print(name, "below", below, "beyond", beyond, "links", sorted(near_links), "dist", np.round(np.sort(dist), 4))
        want = H.MUST_EXERCISE[name]
        assert below >= want[0] and beyond >= want[1] and len(near_links) >= want[2], name
        # the numpy kinematics the picks were made with agree with the oracle's to rounding
        assert np.abs(d.world_points(q[10]) - X[10]).max() < 1e-12
