"""The cases of tests/step_solve_cases.py against their own claims, and the numpy restatement tests/step_solve_ref.py against
the FP64 oracle, before tests/test_gpu_step_solve.py holds the step kernels to both.  No GPU.

  pattern     every case's recorded picks give obstacle blocks at exactly the waypoints D of the case (re-derived from
              Oracle.eval_normal_eq), each voxel an axis neighbour of its point's voxel whose stencil no other waypoint
              touches, and a bound design shows in the census of the iterate it names
  census      the cases together visit every feature of step_solve_cases.REQUIRED
  agreement   the restatement's solve (dense numpy.linalg.solve per step) gives the oracle's iterations, status and accept /
              reject sequence at every cap the GPU test compares, and its iterate within AGREE = 1e-11: a hundred times
              below the GPU tolerance on Q (1e-9).  Measured: 2.4e-13 at most (w8_D4, p12_damping_small); it bounds how
              well two correct FP64 solves of these systems agree.
  decided     every case at every cap, none left out (step_solve_cases.decided)
  teeth       with the coupling e dropped at one structural slot (0, nd - 1, nd, mid - 1, mid, m - 2) the restatement's first
              step moves by at least 1e-6 somewhere: a case that could not show a dropped coupling could not show a wrong
              kernel either
"""
import numpy as np
import pytest

import cull_fields as cf
import step_solve_cases as sc
import step_solve_ref as ref

AGREE = 1e-11


@pytest.mark.parametrize("name", sc.NAMES)
def test_recorded_picks_give_the_chosen_pattern(oracle_mod, name):
    case, p = sc.CASES[name], sc.problem(name)
    assert name in sc.RECORD, "no certificate: PYTHONPATH=. python tests/step_solve_cases.py " + name
    d, geo = p.desc, p.geo
    g, own = geo.grid, sc._owners(geo)
    assert [t for t, _, _ in p.picks] == list(case.D)
    for t, i, cells in p.picks:
        assert d.link_is_moving()[d.point_link[i]]
        v = np.array(cells[0][0])
        assert np.abs(v - geo.pv[0, t, i]).sum() == 1, "not an axis neighbour of the point's voxel"
        assert len(cells) == (2 if t in case.push else 1)
        if t in case.push:
            assert tuple(geo.pv[0, t, i]) == cells[1][0]
        for cv, _ in cells:
            for w in cf._stencil(cv, g):
                assert not own.get(g.flat(w), set()) - {t}, f"waypoint {own[g.flat(w)]} touches the stencil of waypoint {t}'s voxel"
    JtJ, Jtr, _, _, _ = p.o.eval_normal_eq(0, p.goals[None], 1, p.S, p.base, p.Q0[None])
    assert [t for t in range(case.T) if np.any(JtJ[0, t] != 0.0)] == list(case.D)
    assert not np.any(JtJ[0, :2] != 0.0)
    if d.n_opt > 1:
        for t in case.D:
            assert np.any(JtJ[0, t] - np.diag(np.diag(JtJ[0, t])) != 0.0), f"the block of waypoint {t} is diagonal"
    for t in case.push:
        assert Jtr[0, t, p.record["joint"]] * p.record["side"] < 0.0
    feats, first = sc.features(name)
    assert first["obs"] == [t - 2 for t in case.D]
    if case.design:
        want = "frozen_later" if case.design == "late" else case.design
        assert ("wide:" if first["wide"] else "narrow:") + want in feats, feats
        if case.design != "late":
            assert any(x.endswith(want) for x in first["features"]), "a seed design shows at the seed"
    if case.design in sc.PUSH:  # the joint rides on its limit: no velocity gradient, frozen exactly where the field pushes
        j = p.record["joint"]
        assert [s for s in range(first["m"] - 1) if first["act"][s, j]] == [t - 2 for t in case.push]


def test_census_covers_every_feature(oracle_mod):
    table = {}
    for name in sc.NAMES:
        for f in sc.features(name)[0]:
            table.setdefault(f, []).append(name)
    for f in sc.REQUIRED:
        print(f"{f:32s} {' '.join(table.get(f, []))}")
    assert not [f for f in sc.REQUIRED if f not in table]
    # every robot and every width's bound designs are there
    assert {sc.CASES[n].robot for n in sc.NAMES} == set(sc.ROBOTS)


@pytest.mark.parametrize("name", sc.NAMES)
def test_restatement_equals_oracle_and_case_is_decided(oracle_mod, name):
    case, p = sc.CASES[name], sc.problem(name)
    worst = 0.0
    for cap in case.caps:
        Qo, _, fo, ito, sto, acco = sc.oracle_run(name, cap)
        Qr, fr, itr, st, tr = ref.lm(p.o, p, 0, p.Q0, cap)
        assert (itr, st) == (ito, sto), cap
        assert [r["accepted"] for r in tr][:ito] == acco, cap
        worst = max(worst, float(np.abs(Qr - Qo).max()))
        np.testing.assert_allclose(Qr, Qo, rtol=0, atol=AGREE, err_msg=f"cap {cap}")
        np.testing.assert_allclose(fr, fo, rtol=1e-11)
        assert sc.decided(name, cap), f"undecided at cap {cap}: redraw the case"
    # the first trial point itself: the oracle's iterate after one evaluation where the step was accepted
    tr = sc.trace(name)[4]
    if tr[0]["accepted"]:
        np.testing.assert_allclose(tr[0]["trial"], sc.oracle_run(name, 1)[0], rtol=0, atol=AGREE)
    else:
        np.testing.assert_array_equal(sc.oracle_run(name, 1)[0], p.Q0)
    print(f"{name:20s} max |restatement - oracle| over caps {case.caps}: {worst:.2e}")


@pytest.mark.parametrize("name", sc.NAMES)
def test_a_dropped_coupling_shows_in_the_first_step(oracle_mod, name):
    moves = sc.teeth(name)
    print(f"{name:20s} " + " ".join(f"e[{s}]: {v:.1e}" for s, v in moves.items()))
    assert moves, "no structural slot has a coupling left"
    assert min(moves.values()) >= sc.TEETH, moves
