"""Retiming without a GPU: the numpy restatement's controllable sets (tests/retime_ref.py) are what an independent LP
finds, and the robot descriptions carry the URDF's joint velocity limits."""
import json
import os

import numpy as np
import pytest

from grasptrajopt_amd.robot_desc import RobotDesc, load_builtin, with_planar_base
import retime_ref as rr

PANDA_V = [2.175] * 4 + [2.61] * 3 + [0.2] * 2
FETCH_ARM_V = [1.256, 1.454, 1.571, 1.521, 1.571, 2.268, 2.268]


def _random_plan(desc, T, rng):
    """A smooth random plan inside the joint limits; parameter rows constant, as in a solved plan."""
    lo, hi = np.maximum(desc.lower, -3.0), np.minimum(desc.upper, 3.0)
    a, b = lo + (hi - lo) * rng.uniform(0.2, 0.8, desc.ndof), lo + (hi - lo) * rng.uniform(0.2, 0.8, desc.ndof)
    s = np.linspace(0.0, 1.0, T)
    plan = a[:, None] + (b - a)[:, None] * (3 * s ** 2 - 2 * s ** 3)[None, :]
    plan += 0.05 * np.sin(2 * np.pi * rng.uniform(0.5, 2.0, (desc.ndof, 1)) * s[None, :] + rng.uniform(0, 6, (desc.ndof, 1)))
    plan[desc.param_index] = plan[desc.param_index, :1]
    return plan


@pytest.mark.parametrize("robot", ["panda", "fetch_mobile"])
def test_profile_against_lps(robot):
    """The elimination's controllable sets equal an LP's (max x_i over the constraints of gridpoints i..N-1), and the
    profile stays inside them.  The sum-of-x LP over the whole grid is at least as large: the greedy forward pass is
    TOPP-RA's, which is not pointwise maximal where a larger x_i lowers the u_i its segment can take."""
    desc = load_builtin(robot)
    rng = np.random.default_rng(11)
    T = 50 if robot == "panda" else 80
    amax = np.full(desc.ndof, 0.5)
    for _ in range(10):
        plan = _random_plan(desc, T, rng)
        moving = np.any(plan != plan[:, :1], axis=1)
        _, _, p1, p2 = rr.path_derivatives(plan, 2)
        p1[:, ~moving] = 0.0
        p2[:, ~moving] = 0.0
        x, xmax = rr.profile(p1, p2, desc.velocity, amax, moving)
        N = x.shape[0]
        for i in (1, N // 3, N // 2, N - 3):
            xl = rr.controllable_lp(p1, p2, desc.velocity, amax, i)
            assert xmax[i] == pytest.approx(xl, rel=1e-7)
        assert np.all(x <= xmax) and x[0] == 0 and x[-1] == 0
        x_sum = rr.grid_lp(p1, p2, desc.velocity, amax)
        assert x.sum() <= x_sum.sum() * (1 + 1e-9)


def test_restatement_path_is_scipys_spline_through_the_waypoints():
    rng = np.random.default_rng(2)
    desc = load_builtin("panda")
    plan = _random_plan(desc, 9, rng)
    r = rr.retime_one(plan, desc.velocity, np.full(desc.ndof, 0.5), subdiv=3, M=50)
    assert r["status"] == 0 and r["duration"] > 0
    np.testing.assert_allclose(r["q"][0], plan[:, 0], atol=1e-12)
    np.testing.assert_allclose(r["q"][-1], plan[:, -1], atol=1e-12)
    np.testing.assert_allclose(r["qd"][[0, -1]], 0.0, atol=1e-9)
    assert r["t_grid"].shape == (3 * 8 + 1,)


def test_stored_velocity_limits_are_the_urdfs():
    for name in ("panda", "panda_5k"):
        np.testing.assert_array_equal(load_builtin(name).velocity, PANDA_V)
    fetch = load_builtin("fetch")
    np.testing.assert_array_equal(fetch.velocity[fetch.opt_index], FETCH_ARM_V)
    assert fetch.velocity.shape == (15,) and np.all(np.isfinite(fetch.velocity))
    mob = with_planar_base(fetch)
    assert np.all(np.isinf(mob.velocity[:3]))
    np.testing.assert_array_equal(mob.velocity[3:], fetch.velocity)
    assert np.all(np.isinf(load_builtin("fetch_mobile").velocity[:3]))


def test_model_velocity_properties():
    from grasptrajopt_amd.gto_models import GTORobotModel
    m = GTORobotModel(desc=load_builtin("panda"))
    np.testing.assert_array_equal(m.velocity_actuated_joint_limits.toarray().ravel(), PANDA_V)
    np.testing.assert_array_equal(m.velocity_optimized_joint_limits.toarray().ravel(), PANDA_V[:7])
    assert m.velocity_actuated_joint_limits.shape == (9, 1)


def test_velocity_limits_from_urdf():
    from grasptrajopt_amd.urdf import Urdf
    text = """<robot name="r"><link name="a"/><link name="b"/><link name="c"/><link name="d"/>
      <joint name="j1" type="revolute"><parent link="a"/><child link="b"/><limit lower="-1" upper="1" velocity="1.5"/></joint>
      <joint name="j2" type="revolute"><parent link="b"/><child link="c"/><limit lower="-1" upper="1"/></joint>
      <joint name="j3" type="continuous"><parent link="c"/><child link="d"/></joint></robot>"""
    desc = RobotDesc.from_urdf(Urdf.from_string(text), keep_all_frames=True)
    np.testing.assert_array_equal(desc.velocity, [1.5, np.inf, np.inf])


def test_json_without_velocity_key_still_loads(tmp_path):
    desc = load_builtin("panda")
    prefix = str(tmp_path / "panda")
    desc.save(prefix)
    meta = json.load(open(prefix + ".json"))
    assert meta["velocity_limits"] == PANDA_V
    meta.pop("velocity_limits")
    json.dump(meta, open(prefix + ".json", "w"))
    old = RobotDesc.load(prefix)
    assert old.velocity is None and old.ndof == 9
    # null = no limit
    meta["velocity_limits"] = [None] + PANDA_V[1:]
    json.dump(meta, open(prefix + ".json", "w"))
    v = RobotDesc.load(prefix).velocity
    assert np.isinf(v[0]) and v[1] == 2.175
    assert os.path.exists(prefix + ".npz")


def test_restatement_flags_a_plan_that_rests_before_the_end():
    """The profile of this plan reaches x = 0 at gridpoint N-2 (the last segment runs between two zeros): status
    GTO_STATUS_NUMERICAL and NaN samples instead of a duration that round-off decides."""
    desc = load_builtin("panda")
    plans = rr.random_plans(desc, 256, 50, seed=1)
    r = rr.retime(plans[120:123], desc.velocity, np.full(desc.ndof, 0.5))
    assert r["status"].tolist() == [0, rr.GTO_STATUS_NUMERICAL, 0]
    assert np.all(np.isnan(r["q"][1])) and r["sd_grid"][1][-2] <= 1e-3 * r["sd_grid"][1].max()
    assert np.all(r["duration"][[0, 2]] < 10)


def test_tiny_p1_bounds_x_through_the_cap():
    """A p1 so small that amax/|p1| overflows is treated as p1 = 0: |p2 x| <= amax bounds x directly."""
    p1 = np.array([[1.0, 0.0], [1.0, 5e-324], [1.0, 1e-320], [1.0, 0.0]])
    p2 = np.array([[0.0, 0.0], [0.0, 4.0], [0.0, 2.0], [0.0, 0.0]])
    amax = np.array([0.5, 0.5])
    assert rr._has_line(p1[1], p2[1], amax).tolist() == [True, False]
    cap = rr.x_bounds(p1, p2, np.array([np.inf, np.inf]), amax, np.array([True, True]))
    assert cap[1] == 0.125 and cap[2] == 0.25
