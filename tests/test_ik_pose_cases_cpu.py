"""The case table of tests/ik_pose_cases.py without a GPU: that it reaches every branch of ik_orient_goal_wave's pose
arithmetic (on the oracle's frames), the host's goal conversions against the restatement at every case pose, the
restatement's gradient against central differences up to the clamp, and each case's sensitivity allowance."""
import numpy as np
import pytest

import ik_pose_cases as ipc
import ik_pose_ref as ref

Q, RPY = ref.GTO_IK_GOAL_QUATERNION, ref.GTO_IK_GOAL_RPY


@pytest.fixture(scope="module")
def tab(oracle_mod):
    desc, o, opts, cases = ipc.table(oracle_mod)
    fe = desc.frame_index(ipc.EE)
    frames = o.eval_fk(np.stack([ipc.clipped(desc, c.q0) for c in cases]))
    return desc, o, opts, cases, {c.name: frames[i, fe] for i, c in enumerate(cases)}, frames


def _cut_distance(R):
    return min(abs(abs(a) - np.pi) for a in ref.rpy_of(R)[[0, 2]])


def _sq(R):
    return np.sqrt(max(0.0, 1.0 - R[2, 0] ** 2))


def test_robot_is_a_gimbal(tab):
    desc, o, opts, cases, T, frames = tab
    assert desc.n_opt == 7 and list(desc.param_index) == [ipc.J_TAB] and np.all(desc.origin_rpy[[0, 1, 2, 3, 6, 7, 8, 9]] == 0)
    for i, c in enumerate(cases):
        np.testing.assert_allclose(T[c.name], ipc.gimbal_pose(ipc.clipped(desc, c.q0)), rtol=0, atol=1e-15)
        R, q = T[c.name][:3, :3], c.q0
        assert R[2, 0] == -np.sin(q[ipc.PITCH])  # row 2 of Rz Ry Rx meets only exact zeros and ones
        if abs(q[ipc.PITCH]) < np.pi / 2 and not c.on_clamp:
            np.testing.assert_allclose(ref.rpy_of(R), q[[ipc.ROLL, ipc.PITCH, ipc.YAW]], rtol=0, atol=1e-15 / _sq(R) ** 2)
        S = ref.screws(desc, frames[i], desc.frame_index(ipc.EE))
        moving = np.abs(S).sum(axis=1) > 0
        assert sum(int(m) << j for j, m in enumerate(moving)) == ipc.ANC_EE and not moving[ipc.OPT_FLAP]
    beyond = np.abs(np.stack([c.q0 for c in cases])[:, desc.opt_index]) > desc.upper[desc.opt_index]
    assert [c.name for c, b in zip(cases, beyond.any(axis=1)) if b] == ["q_clip", "q_clip_neg"]  # the others never clip
    assert beyond[[c.name for c in cases].index("q_clip")].tolist() == [True, False, False, True, False, False, False]
    assert np.all(np.abs(np.stack([c.goal[:3] for c in cases])) < 0.5)  # within reach of the prismatic joints


def test_quaternion_coverage(tab):
    desc, o, opts, cases, T, _ = tab
    qc = [c for c in cases if c.kind == Q]
    hits = np.zeros(4, dtype=int)
    for c in qc:
        R = T[c.name][:3, :3]
        if c.cls == "branch":
            assert ref.shepperd_margin(R) >= 0.05, c
            assert ref.shepperd_branch(R) == "wxyz".index(c.name[2]), c
            hits[ref.shepperd_branch(R)] += 1
    assert np.all(hits >= 3), hits
    R = T["q_boundary"][:3, :3]
    tr = np.trace(R)
    assert abs(tr - R[0, 0]) < 1e-9 and abs(R[0, 0] - R[1, 1]) < 1e-9
    P = ipc.PERMUTATION
    assert np.trace(P) == P[0, 0] == 0 and np.array_equal(P @ P @ P, np.eye(3)) and np.linalg.det(P) == 1.0
    by = {c.name: c for c in cases}
    assert np.array_equal(by["q_perm_goal"].goal_pose[:3, :3], P)
    np.testing.assert_allclose(T["q_perm_seed"][:3, :3], P, rtol=0, atol=2e-16)
    for name, D, j in (("q_x_diag", (1, -1, -1), ipc.ROLL), ("q_y_diag", (-1, 1, -1), ipc.PITCH), ("q_z_diag", (-1, -1, 1), ipc.YAW)):
        assert np.array_equal(np.diag(T[name][:3, :3]), D) and by[name].q0[j] == np.pi
        assert np.count_nonzero(by[name].q0[[ipc.YAW, ipc.PITCH, ipc.ROLL]]) == 1
        np.testing.assert_allclose(T[name][:3, :3], np.diag(D), rtol=0, atol=2e-16)
    norms = {c.name: np.linalg.norm(c.goal[3:]) for c in qc}
    unit = [c for c in qc if abs(norms[c.name] - 1.0) < 1e-15]
    assert any(c.goal[6] < 0 for c in unit) and any(c.goal[6] > 0 for c in unit)
    assert abs(norms["q_scaled_half"] - 0.5) < 1e-15 and abs(norms["q_scaled_double"] - 2.0) < 1e-15 and norms["q_zero"] == 0.0
    for c in unit:  # every unit goal and its negative are both in the table
        assert any(o_.q0 is c.q0 and np.array_equal(o_.goal[:3], c.goal[:3]) and np.array_equal(o_.goal[3:], -c.goal[3:]) for o_ in unit), c
    for c in qc:
        if c.twin:
            assert np.array_equal(by[c.twin].goal[3:], -c.goal[3:]) and by[c.twin].q0 is c.q0
    assert any(c.goal_pose is not None for c in qc) and any(c.goal_pose is None and c.cls == "branch" for c in qc)


def test_rpy_coverage(tab):
    desc, o, opts, cases, T, _ = tab
    rc = [c for c in cases if c.kind == RPY]
    graded = {(np.sign(c.q0[ipc.PITCH]), c.d) for c in rc if c.cls == "graded"}
    assert graded == {(s, d) for s in (1.0, -1.0) for d in (1e-1, 1e-2, 1e-3, 1e-4, 1e-6)}
    for c in rc:
        if c.cls == "graded":
            assert abs(c.q0[ipc.PITCH]) == np.pi / 2 - c.d and abs(T[c.name][2, 0]) < 1.0
    clamp = sorted(T[c.name][2, 0] for c in rc if c.cls == "clamp")
    assert clamp == [-1.0, 1.0]
    assert all(ref.rpy_of(T[c.name][:3, :3])[1] == np.pi / 2 for c in rc if c.cls == "clamp")  # (+pi/2 at R20 = +1 too)
    seen = set()
    for c in rc:
        if c.cls != "cut":
            continue
        for j, k, tag in ((ipc.YAW, 5, "yaw"), (ipc.ROLL, 3, "roll")):
            if abs(c.q0[j]) > 3.0:
                assert abs(c.q0[j]) == np.pi - c.d
                on_cut = abs(c.goal[k]) == np.pi
                seen.add((tag, np.sign(c.q0[j]), c.d, "cut" if on_cut else ("same" if c.goal[k] * c.q0[j] > 0 else "other")))
                assert _cut_distance(T[c.name][:3, :3]) == pytest.approx(c.d, rel=1e-6)
    for tag in ("yaw", "roll"):
        for s in (1.0, -1.0):
            assert (tag, s, 1e-2, "cut") in seen
            for d in (1e-2, 1e-6):
                assert (tag, s, d, "same") in seen and (tag, s, d, "other") in seen
    assert any(c.goal_pose is not None for c in rc) and any(c.goal_pose is None for c in rc)


def test_host_conversions_match_restatement(tab):
    from grasptrajopt_amd import utils
    desc, o, opts, cases, T, _ = tab
    poses = [T[c.name][:3, :3] for c in cases] + [c.goal_pose[:3, :3] for c in cases if c.goal_pose is not None]
    n_cut = n_clamp = 0
    for R in poses:
        w, x, y, z = utils.mat2quat(R)
        q, want = np.array([x, y, z, w]), ref.quat_of(R)
        assert min(np.abs(q - want).max(), np.abs(q + want).max()) < 1e-12
        got, rpy = utils.quat2rpy(x, y, z, w), ref.rpy_of(R)
        if abs(R[2, 0]) >= 1.0:  # on the clamp roll and yaw are atan2 of rounding noise: only pitch is defined; through the
            n_clamp += 1         # quaternion sin(pitch) is 1 to a few ulp, and asin turns an ulp into sqrt(2 ulp) = 2e-8
            assert abs(got[1] - rpy[1]) < 1e-7
        elif _sq(R) >= 1e-3:
            if _cut_distance(R) < 1e-12:  # on an atan2 cut +-pi is the sign of a rounded zero
                n_cut += 1
                np.testing.assert_allclose(np.abs(got), np.abs(rpy), rtol=0, atol=1e-12)
            else:
                np.testing.assert_allclose(got, rpy, rtol=0, atol=1e-12)
    assert n_clamp >= 2 and n_cut >= 3
    for c in cases:
        if c.goal_pose is not None:
            conv = utils.ik_goal_quaternion if c.kind == Q else utils.ik_goal_rpy
            assert np.array_equal(c.goal if c.twin is None else np.concatenate([c.goal[:3], -c.goal[3:]]), conv(c.goal_pose))


def test_gradient_matches_central_differences_up_to_the_clamp(tab):
    """The check tests/test_ik_pose_cpu.py skips near the clamp: the step shrinks and the tolerance grows with
    sqrt(1 - R20^2), the scale on which the angles' derivatives change."""
    desc, o, opts, cases, T, _ = tab
    oi, checked, near = desc.opt_index, 0, 0
    for c in cases:
        R = T[c.name][:3, :3]
        if c.on_clamp or (c.kind == RPY and _cut_distance(R) < 1e-2 - 1e-12):  # (pi - (pi - 1e-2) as it rounds)
            continue
        sq = _sq(R) if c.kind == RPY else 1.0
        x = ipc.clipped(desc, c.q0)[oi]
        prob = ipc.problem(o, desc, c)
        f0, b, A = prob.eval(x)
        h = 1e-6 * sq
        grad = np.array([(prob.f(x + h * e)[0] - prob.f(x - h * e)[0]) / (2 * h) for e in np.eye(len(x))])
        # the differences' own rounding: R20 is rounded to eps, which asin turns into eps / sq of pitch, so each value is
        # uncertain by 2 |r| / pi * eps / sq / pi and their difference over 2 h by that over h (1e-12 at sq = 1e-6, where
        # h = 1e-12 is below the 1e-10 to which pitch can be told from R20 at all)
        r, _ = ref.residual(c.kind, T[c.name], c.goal)
        noise = 0.0 if c.kind == Q else 2.0 * np.abs(r[3:]).max() / np.pi ** 2 * np.finfo(float).eps / sq / h
        np.testing.assert_allclose(2 * b, grad, rtol=1e-6 / sq, atol=1e-8 * max(1.0, np.abs(grad).max()) + noise, err_msg=c.name)
        assert b[ipc.OPT_FLAP] == 0.0 and np.all(A[ipc.OPT_FLAP] == 0.0) and np.all(A[:, ipc.OPT_FLAP] == 0.0)
        assert np.allclose(A, A.T) and np.linalg.eigvalsh(A).min() > -1e-12 * np.abs(A).max()
        checked += 1
        near += sq < 1e-2
    assert checked >= 50 and near >= 4


def test_zero_quaternion_goal_has_no_orientation_rows(tab):
    desc, o, opts, cases, T, frames = tab
    i = [c.name for c in cases].index("q_zero")
    c = cases[i]
    J = ref.jacobian(Q, T[c.name], c.goal, ref.screws(desc, frames[i], desc.frame_index(ipc.EE)))
    assert np.all(J[3:] == 0.0) and np.abs(J[:3]).max() > 0.1
    assert ref.pose_term(Q, T[c.name], c.goal) == np.sum((T[c.name][:3, 3] - c.goal[:3]) ** 2) + 1.0


def test_allowances_and_lockstep_list(tab):
    """Each case's allowance (the restatement alone, frames turned by +-ETA) and who is left out of the lock-step test."""
    desc, o, opts, cases, T, _ = tab
    assert ipc.ETA == 1e-13  # tests/test_gpu_parity.py::test_fk_matches_golden_and_oracle: eval_fk against the oracle
    for c in cases:
        step = "-" if c.allow_step is None else f"{c.allow_step:.3e}"
        print(f"{c.name:24s} {c.cls:11s} lock-step {int(c.lockstep)}  allowance: value {c.allow_value:.3e}  one step {step}")
        assert np.isfinite(c.allow_value) and (c.on_clamp or np.isfinite(c.allow_step))
    off = [c for c in cases if not c.on_clamp]
    print(f"largest allowance off the clamp: value {max(c.allow_value for c in off):.3e} one step {max(c.allow_step for c in off):.3e}; "
          f"among the lock-step cases: value {max(c.allow_value for c in off if c.lockstep):.3e} "
          f"one step {max(c.allow_step for c in off if c.lockstep):.3e}")
    eligible = [c for c in cases if c.lockstep or c.name in ipc.LOCKSTEP_LEFT_OUT]
    assert all(c.cls in ("branch", "boundary", "permutation", "scaled", "zero", "clipped") or c.d >= (1e-3 if c.cls == "graded" else 1e-2)
               for c in eligible)
    assert 10 * len(ipc.LOCKSTEP_LEFT_OUT) <= len(eligible)
    by = {c.name: c for c in cases}
    for name in ipc.LOCKSTEP_LEFT_OUT:
        assert ipc.unstable(o, opts, desc, by[name]), name
    # the first step of every pivot case is taken: a wrong Jacobian row would move it
    for c in cases:
        if c.cls == "branch":
            q1, _, it, st = ref.solve(ipc.problem(o, desc, c), c.q0, opts, 1)
            assert (it, st) == (1, ref.GTO_STATUS_MAX_ITER) and np.abs(q1 - c.q0).max() > 0.1
            assert q1[ipc.J_FLAP] == c.q0[ipc.J_FLAP] and q1[ipc.J_TAB] == c.q0[ipc.J_TAB]
