"""CPU: the oracle and the cases of tests/solver_opts_cases.py, judged before they judge a kernel.

The oracle is pinned to the reference's fixtures at the reference's constants only.  Here its objective terms are held to a
numpy restatement (solver_opts_cases.independent_terms) under every option set, and to the scaling laws the terms obey; the
option sets are held to what they claim (each moves the solution by 100 times what the GPU comparison allows, runs_to_cap
ends at the cap, ends_by_step ends through the step tolerance); and the "decided" filter is held to its cap.

Decided: an instance is compared on the GPU only if the oracle alone gives the same iteration count and status, and its
answer within 1e-9, when the seed's optimised entries are moved by +-1e-13.  At most one instance in eight of an (option
set, problem) may be left out, none on `reference` and `runs_to_cap`.  With the instances picked in solver_opts_cases.py
none is left out anywhere; the test prints the list per option set all the same.
"""
import numpy as np
import pytest

import solver_opts_cases as soc

STATUS_CONVERGED, STATUS_MAX_ITER, STATUS_NUMERICAL = 0, 1, 2
FIELDS = ("w_obstacle", "w_vel", "Tmax", "lambda0", "tol_step")
OTHERS = [n for n in soc.NAMES if n != "reference"]


def test_option_sets_move_every_field_the_suite_kept_constant(oracle_mod):
    ref = soc.opts_of(oracle_mod, "reference")
    d = oracle_mod.reference_opts()
    assert all(getattr(ref, f) == getattr(d, f) for f in FIELDS + ("tol_rel_f",))
    for f in FIELDS:
        moved = [n for n in OTHERS if getattr(soc.opts_of(oracle_mod, n), f) != getattr(ref, f)]
        assert len(moved) >= 2, f
    m = soc.opts_of(oracle_mod, "mixed")
    assert all(getattr(m, f) != getattr(ref, f) for f in FIELDS)
    dt = lambda o: o.Tmax / (o.T - 1)
    alpha = lambda o: o.w_vel / dt(o) ** 2
    np.testing.assert_allclose(alpha(soc.opts_of(oracle_mod, "time_short")) / alpha(ref), 400.0, rtol=1e-12)
    assert alpha(soc.opts_of(oracle_mod, "velocity_off")) == 0.0


@pytest.mark.parametrize("key", list(soc.TRAJ))
def test_oracle_terms_match_numpy_under_every_option_set(oracle_mod, key):
    """f_goal, f_obs, f_vel of the oracle against numpy with the same options (1e-10 relative, the suite's tolerance for
    objective terms), and against the oracle at `reference` through the scaling laws (1e-14 relative: a few roundings)."""
    p = soc.traj_problem(oracle_mod, key)
    ref_o = soc.opts_of(oracle_mod, "reference")
    o_ref = soc.oracle_for(oracle_mod, p, ref_o)
    args = (soc.DENSE, p.goals, p.n_goals, p.S, p.base, p.Q_eval)
    fg0, fo0, fv0, am0 = o_ref.eval_objective(*args)
    assert (fg0 > 0).all() and (fv0 > 0).all() and (fo0 > 0).all(), "the trajectory leaves a term at zero"
    for name in soc.NAMES:
        opts = soc.opts_of(oracle_mod, name)
        o = soc.oracle_for(oracle_mod, p, opts)
        fg, fo, fv, am = o.eval_objective(*args)
        ig, io, iv, iam = soc.independent_terms(o, p, opts, p.Q_eval, sid=soc.DENSE)
        np.testing.assert_allclose(fg, ig, rtol=1e-10, atol=0, err_msg=name)
        np.testing.assert_allclose(fo, io, rtol=1e-10, atol=0, err_msg=name)
        np.testing.assert_allclose(fv, iv, rtol=1e-10, atol=0, err_msg=name)
        np.testing.assert_array_equal(am, iam)
        np.testing.assert_array_equal(fg, fg0)
        np.testing.assert_array_equal(am, am0)
        np.testing.assert_allclose(fo, fo0 * (opts.w_obstacle / ref_o.w_obstacle), rtol=1e-14, atol=0, err_msg=name)
        np.testing.assert_allclose(fv, fv0 * (opts.w_vel / ref_o.w_vel) * (ref_o.Tmax / opts.Tmax) ** 2, rtol=1e-14, atol=0, err_msg=name)


@pytest.mark.parametrize("key", list(soc.TRAJ))
def test_every_option_set_moves_the_solution(oracle_mod, key):
    """The oracle's solved Q differs from its `reference` result by at least 1e-4 rad somewhere, or f by at least 1e-5
    relative: 100 times what the GPU comparison allows (1e-6 rad, 1e-7), so a kernel that ignored the option cannot pass.
    Where Q may barely move (ends_by_step, runs_to_cap) the iteration counts differ on most instances."""
    Qr, _, fr, itr, _ = soc.traj_oracle(oracle_mod, key, "reference")
    for name in OTHERS:
        Q, _, f, it, st = soc.traj_oracle(oracle_mod, key, name)
        dq, df = np.abs(Q - Qr).max(), (np.abs(f - fr) / np.abs(fr)).max()
        print(f"{key:18s} {name:15s} max|Q - Q_reference| {dq:.3e}  max rel |f - f_reference| {df:.3e}  iterations differ on "
              f"{int((it != itr).sum())} of {len(it)}")
        assert dq >= 1e-4 or df >= 1e-5, name
        if name in ("ends_by_step", "runs_to_cap"):
            assert (it != itr).sum() * 2 > len(it), name


@pytest.mark.parametrize("key", list(soc.TRAJ))
def test_endings(oracle_mod, key):
    """runs_to_cap: GTO_STATUS_MAX_ITER at exactly the cap on every instance.  ends_by_step: converged below the cap, and
    with tol_step = 0 (tol_rel_f is 0 in that set already) the counts change: the step test was what ended the solve.
    velocity_off: the oracle ends GTO_STATUS_NUMERICAL before its first step, the seed returned as it is (alpha = 0 leaves
    the free waypoints without goal or obstacle rows with blocks of exact zeros, which Marquardt's scaling of the diagonal
    does not damp: the block solve refuses the zero pivot).  The GPU must do the same."""
    _, _, _, it, st = soc.traj_oracle(oracle_mod, key, "runs_to_cap")
    assert (st == STATUS_MAX_ITER).all() and (it == soc.SMALL_CAP).all()
    _, _, _, it, st = soc.traj_oracle(oracle_mod, key, "ends_by_step")
    assert (st == STATUS_CONVERGED).all() and (it < soc.CAP).all()
    _, _, _, it0, st0 = soc.traj_oracle(oracle_mod, key, "ends_by_step", tol_step=0.0)
    assert (it0 > it).all()  # (then to the cap, or until the damping overflows on a point without a descent direction)
    p = soc.traj_problem(oracle_mod, key)
    Q, dQ, f, it, st = soc.traj_oracle(oracle_mod, key, "velocity_off")
    assert (st == STATUS_NUMERICAL).all() and (it == 0).all() and np.isfinite(f).all()
    oi = p.desc.opt_index
    np.testing.assert_array_equal(Q[:, oi, 2:], np.clip(p.Q0[:, oi, 2:], p.desc.lower[oi][None, :, None], p.desc.upper[oi][None, :, None]))
    # the other sets reach their endings through more than one branch between them
    sts = np.concatenate([soc.traj_oracle(oracle_mod, key, n)[4] for n in soc.NAMES])
    assert set(sts.tolist()) == {STATUS_CONVERGED, STATUS_MAX_ITER, STATUS_NUMERICAL}


@pytest.mark.parametrize("name", soc.NAMES)
def test_decided_filter_stays_within_its_cap(oracle_mod, name):
    """Every (option set, problem) of every solver the GPU file compares; the capped trajectory solves (1 and 2 iterations)
    included."""
    rows = []
    for key in soc.TRAJ:
        for kw in ({}, {"max_iter": 1}, {"max_iter": 2}):
            rows.append((f"trajectory {key} {kw or ''}", soc.traj_decided(oracle_mod, key, name, **kw)))
    for robot in soc.IK_ROBOTS:
        for collide in (False, True):
            rows.append((f"ik {robot} scene={collide}", soc.ik_oracle(oracle_mod, robot, name, collide)[1]))
            rows.append((f"lift {robot} scene={collide}", soc.lift_oracle(oracle_mod, robot, name, collide)[1]))
    rows.append(("base fetch", soc.base_oracle(oracle_mod, name)[1]))
    rows.append(("pose gimbal", soc.pose_oracle(oracle_mod, name)[1]))
    for what, dec in rows:
        print(f"{name:15s} {what:45s} left out {np.flatnonzero(~dec).tolist()} of {len(dec)}")
    for what, dec in rows:
        assert soc.within_cap(name, dec), (what, np.flatnonzero(~dec).tolist())


def _bits(res):
    return tuple(np.ascontiguousarray(x).tobytes() for x in res)


def test_other_solvers_read_the_fields_they_should_and_no_others(oracle_mod):
    """IK (and the retrieve lift built on it) reads w_obstacle (with a scene), lambda0 and the tolerances; base placement
    lambda0 and the tolerances.  w_vel and Tmax belong to the trajectory solve alone: they leave the oracle's IK and base
    results bit-identical, and so does w_obstacle without a scene and for the base solve.  The sets that should matter do."""
    inert = ("velocity_stiff", "velocity_off", "time_short", "time_long")
    for robot in soc.IK_ROBOTS:
        for collide in (False, True):
            ref = _bits(soc.ik_oracle(oracle_mod, robot, "reference", collide)[0])
            for name in inert + (() if collide else ("obstacle_heavy", "obstacle_off")):
                assert _bits(soc.ik_oracle(oracle_mod, robot, name, collide)[0]) == ref, (robot, collide, name)
            for name in ("damping_small", "damping_large", "ends_by_step", "runs_to_cap", "mixed") + (("obstacle_heavy", "obstacle_off") if collide else ()):
                assert _bits(soc.ik_oracle(oracle_mod, robot, name, collide)[0]) != ref, (robot, collide, name)
    ref = _bits(soc.base_oracle(oracle_mod, "reference")[0])
    for name in inert + ("obstacle_heavy", "obstacle_off"):
        assert _bits(soc.base_oracle(oracle_mod, name)[0]) == ref, name
    for name in ("damping_small", "damping_large", "ends_by_step", "runs_to_cap", "mixed"):
        assert _bits(soc.base_oracle(oracle_mod, name)[0]) != ref, name
    # endings of the other solvers
    for res in [soc.ik_oracle(oracle_mod, r, "runs_to_cap", c)[0] for r in soc.IK_ROBOTS for c in (False, True)]:
        assert (res[2] == soc.SMALL_CAP).all() and (res[3] == STATUS_MAX_ITER).all()
    for res in [soc.ik_oracle(oracle_mod, r, "ends_by_step", c)[0] for r in soc.IK_ROBOTS for c in (False, True)]:
        assert (res[3] == STATUS_CONVERGED).all() and (res[2] < 50).all()
    y, q, f, it, st = soc.base_oracle(oracle_mod, "runs_to_cap")[0]
    assert (it == soc.SMALL_CAP).all() and (st == STATUS_MAX_ITER).all()
    y, q, f, it, st = soc.base_oracle(oracle_mod, "ends_by_step")[0]
    assert (st == STATUS_CONVERGED).all() and (it < soc.BASE_CAP).all()
