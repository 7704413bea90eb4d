"""Orientation-goal IK without a GPU: the host's goal conversions (utils.mat2quat / quat2rpy) and the numpy restatement
of the pose terms (tests/ik_pose_ref.py) against the reference's own arithmetic (tests/golden/ik_pose.npz, written by
tests/golden/make_ik_pose_golden.py), and the restatement's Jacobian against central differences of its value."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT, golden
import ik_pose_ref as ref

ROBOTS = ["panda", "fetch"]


@pytest.fixture(scope="module")
def fx():
    return golden("ik_pose.npz")


def _kin(oracle_mod, robot):
    from grasptrajopt_amd.robot_desc import load_builtin
    cfg = json.load(open(os.path.join(ROOT, "grasptrajopt_amd", "data", f"{robot}_cfg.json")))
    d = load_builtin(robot)
    return d, cfg, oracle_mod.Oracle(d, cfg["link_ee"], cfg["link_gripper"])


def test_new_modules_import():
    from grasptrajopt_amd import ik_solver_quaternion, ik_solver_rpy
    assert ik_solver_quaternion.IKSolver.GOAL_KIND == 1 and ik_solver_rpy.IKSolver.GOAL_KIND == 2


@pytest.mark.parametrize("robot", ROBOTS)
def test_fixture_has_the_clamp_cases(fx, robot):
    kind = fx[f"{robot}_kind"]
    assert (kind == 0).sum() == 64 and (kind == 1).sum() >= 2
    assert (fx["panda_kind"] == 2).sum() + (fx["fetch_kind"] == 2).sum() >= 1
    onc = kind == 2
    assert np.all(fx[f"{robot}_rpy"][onc, 1] == np.pi / 2)


@pytest.mark.parametrize("robot", ROBOTS)
def test_mat2quat_matches_reference_quaternion(fx, oracle_mod, robot):
    from grasptrajopt_amd import utils
    d, cfg, o = _kin(oracle_mod, robot)
    fr = o.eval_fk(fx[f"{robot}_q"])[:, d.frame_index(cfg["link_ee"])]
    np.testing.assert_allclose(fr[:, :3, 3], fx[f"{robot}_pos"], rtol=0, atol=1e-12)
    for i, T in enumerate(fr):
        w, x, y, z = utils.mat2quat(T[:3, :3])
        q = np.array([x, y, z, w])
        r = fx[f"{robot}_quat"][i]
        assert min(np.abs(q - r).max(), np.abs(q + r).max()) < 1e-12, (i, q, r)
        assert min(np.abs(ref.quat_of(T[:3, :3]) - r).max(), np.abs(ref.quat_of(T[:3, :3]) + r).max()) < 1e-12


@pytest.mark.parametrize("robot", ROBOTS)
def test_quat2rpy_and_pose_terms_match_reference(fx, oracle_mod, robot):
    from grasptrajopt_amd import utils
    d, cfg, o = _kin(oracle_mod, robot)
    fr = o.eval_fk(fx[f"{robot}_q"])[:, d.frame_index(cfg["link_ee"])]
    for i, T in enumerate(fr):
        np.testing.assert_allclose(utils.quat2rpy(*fx[f"{robot}_quat"][i]), fx[f"{robot}_rpy_of_quat"][i], rtol=0, atol=1e-12)
        if fx[f"{robot}_kind"][i] == 2:  # on the clamp roll and yaw are atan2 of rounding noise: only pitch is defined
            assert ref.rpy_of(T[:3, :3])[1] == fx[f"{robot}_rpy"][i][1] == np.pi / 2
            continue
        got, want_rpy = ref.rpy_of(T[:3, :3]), fx[f"{robot}_rpy"][i]
        if np.any(np.abs(np.abs(want_rpy[[0, 2]]) - np.pi) < 1e-12):  # on an atan2 cut: +-pi is the sign of a rounded zero
            np.testing.assert_allclose(np.abs(got), np.abs(want_rpy), rtol=0, atol=1e-12)
            continue
        np.testing.assert_allclose(got, want_rpy, rtol=0, atol=1e-12)
        for kind, key in ((ref.GTO_IK_GOAL_QUATERNION, "quat"), (ref.GTO_IK_GOAL_RPY, "rpy")):
            g = fx[f"{robot}_goal_{key}"][i]
            want = fx[f"{robot}_f_{key}"][i]
            assert abs(ref.pose_term(kind, T, g) - want) <= 1e-12 * max(1.0, abs(want)), (kind, i)


def test_fromrpy_composition_pinned(fx):
    """The reference's Quaternion.fromrpy of the fixed-joint rotations is the quaternion of rpy2r's matrix."""
    from grasptrajopt_amd.gto_models import _rpy2r
    for r, qv in zip(fx["panda_rpy_samples"], fx["panda_fromrpy"]):
        q = ref.quat_of(_rpy2r(r))
        assert min(np.abs(q - qv).max(), np.abs(q + qv).max()) < 1e-12


def test_goal_vectors_as_the_reference_builds_them(fx, oracle_mod):
    from grasptrajopt_amd import utils
    d, cfg, o = _kin(oracle_mod, "panda")
    T = o.eval_fk(fx["panda_q"][:8])[:, d.frame_index(cfg["link_ee"])]
    for i in range(8):
        gq = utils.ik_goal_quaternion(T[i])
        assert gq.shape == (7,) and gq[6] >= 0 and np.allclose(gq[:3], T[i][:3, 3])
        np.testing.assert_allclose(abs(gq[3:] @ fx["panda_quat"][i]), 1.0, atol=1e-12)
        np.testing.assert_allclose(utils.ik_goal_rpy(T[i])[3:], fx["panda_rpy"][i], atol=1e-12)


@pytest.mark.parametrize("robot", ROBOTS)
@pytest.mark.parametrize("kind", [ref.GTO_IK_GOAL_QUATERNION, ref.GTO_IK_GOAL_RPY])
def test_jacobian_matches_central_differences(fx, oracle_mod, robot, kind):
    d, cfg, o = _kin(oracle_mod, robot)
    key = "quat" if kind == ref.GTO_IK_GOAL_QUATERNION else "rpy"
    oi = d.opt_index
    checked = 0
    for i in np.nonzero(fx[f"{robot}_kind"] == 0)[0][:24]:
        q = fx[f"{robot}_q"][i]
        x = np.clip(q[oi], d.lower[oi], d.upper[oi])
        g = fx[f"{robot}_goal_{key}"][i]
        prob = ref.PoseProblem(o, d, cfg["link_ee"], kind, q, g)
        T = prob.frames(x[None])[0][prob.fe]
        R = T[:3, :3]
        if kind == ref.GTO_IK_GOAL_RPY and (1 - abs(R[2, 0]) < 1e-3 or abs(R[2, 1]) < 1e-3 > R[2, 2] or
                                             min(abs(abs(a) - np.pi) for a in ref.rpy_of(R)[[0, 2]]) < 1e-2):
            continue  # away from the clamp and the atan2 cuts
        f0, b, A = prob.eval(x)
        h = 1e-6
        grad = np.array([(prob.f(x + h * e)[0] - prob.f(x - h * e)[0]) / (2 * h) for e in np.eye(len(x))])
        np.testing.assert_allclose(2 * b, grad, rtol=1e-6, atol=1e-8 * max(1.0, np.abs(grad).max()))
        assert np.allclose(A, A.T) and np.linalg.eigvalsh(A).min() > -1e-12
        checked += 1
    assert checked >= 12
