"""GPU: the crew at the end of the itemized obstacle launch's grid.

A round that fills the GPU lays its itemized k_obstacle_gram launch out over an ESTIMATE of the item list's length; the
last GTO_SWEEP_WGS (64) workgroups of the same grid are the crew that walks whatever the estimate missed, in steps of 64.
GTO_ITEM_HINT fixes the estimate, so the overflow can be made any size: every item must be evaluated by exactly one
workgroup with the same arithmetic whether it falls to a regular workgroup or to the crew, hence every output of the call
is the same bits for any estimate (assert_array_equal throughout; the oracle at the tolerances of test_gpu_parity.py:
iteration counts equal, trajectories within 1e-6 rad).

The problems are the smallest on which itemized rounds run at all: 160 instances of the Panda with 5 k surface points
(GTO_FEW_INSTANCES=64 keeps the call out of the few-instance launches), and a horizon of five waypoints, where a job is
one waypoint group."""
import numpy as np
import pytest

from helpers import Problem

pytestmark = pytest.mark.gpu

K_OBS, K_STEP = "k_obstacle_gram<8,1>", "k_lm_step<4,1>"
MAX_ITER = 40
# estimates of the item list's length: 8 -- everything falls to the crew, whose workgroups loop; 16, 64, 72, 136 -- the
# crew's 64 workgroups loop more than once / once / partly; 300 -- an overflow of fewer than 64 items or none at all
HINTS = (8, 16, 64, 72, 136, 300)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


def new_handle(capi, oracle_mod, prob, env, **opt_kw):
    """A handle created under `env` (the library reads its knobs when a handle is created) on top of GTO_FEW_INSTANCES=64."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("GTO_FEW_INSTANCES", "64")
        for k in ("GTO_ITEM_HINT", "GTO_SLOTS", "GTO_PREBROAD", "GTO_ITEM_GRID"):
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        h = capi.SolverHandle(prob.desc, prob.cfg["link_ee"], prob.cfg["link_gripper"], oracle_mod.reference_opts(**opt_kw), device=0)
        h.set_mode(0)
        if getattr(prob, "goals", None) is None:
            prob.finish(h.eval_fk)
        h.set_scene(*prob.scene_args())
    return h


def solve(capi, oracle_mod, prob, env, profile=False, lanes=None, **opt_kw):
    """(outputs, kernel profile or None) of one call on a fresh handle."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("GTO_FEW_INSTANCES", "64")  # (also read when a call starts)
        for k, v in env.items():
            mp.setenv(k, v)
        h = new_handle(capi, oracle_mod, prob, env, **opt_kw)
        if lanes is not None:
            h.set_lanes(*lanes)
        h.set_profiling(profile)
        out = h.solve_batch(*prob.solve_args())
        prof = h.last_kernel_profile() if profile else None
        h.close()
    return out, prof


@pytest.fixture(scope="module")
def first_shape(capi, oracle_mod):
    """The shape of test_step_kernel_broad_phase_does_not_change_results and its reference run: no GTO_ITEM_HINT, profiled."""
    prob = Problem("panda_5k", B=160, scene_seed=5, n=64, res=0.035, n_goals=1)
    ref, prof = solve(capi, oracle_mod, prob, {}, profile=True, max_iter=MAX_ITER)
    for a in ref:
        a.setflags(write=False)
    return prob, ref, prof


def assert_same(ref, got):
    for a, b in zip(ref, got):  # Q, dQ, cost, iterations, status
        np.testing.assert_array_equal(a, b)


def test_reference_run_matches_oracle(capi, oracle_mod, first_shape):
    prob, ref, prof = first_shape
    assert prof[K_STEP][1] > 10, prof  # itemized rounds ran
    o = oracle_mod.Oracle(prob.desc, prob.cfg["link_ee"], prob.cfg["link_gripper"], oracle_mod.reference_opts(max_iter=MAX_ITER))
    o.set_scene(*prob.scene_args())
    sub = slice(0, 12)
    args = list(prob.solve_args())
    Qo, dQo, fo, ito, sto = o.solve_batch(args[0], args[1][sub], args[2][sub], args[3], args[4], args[5][sub], args[6][sub])
    np.testing.assert_array_equal(ref[3][sub], ito)
    np.testing.assert_allclose(ref[0][sub], Qo, rtol=0, atol=1e-6)


@pytest.mark.parametrize("slots", [None, "96"])
@pytest.mark.parametrize("hint", HINTS)
def test_crew_range_covers_every_overflow_size(capi, oracle_mod, first_shape, hint, slots):
    """Any estimate, with and without refills in mid-call (96 positions for 160 instances), gives the reference's bits; the
    reference's first 12 instances equal the oracle's (test_reference_run_matches_oracle)."""
    prob, ref, _ = first_shape
    env = {"GTO_ITEM_HINT": str(hint)}
    if slots:
        env["GTO_SLOTS"] = slots
    got, _ = solve(capi, oracle_mod, prob, env, max_iter=MAX_ITER)
    assert_same(ref, got)


def test_crew_did_real_work(capi, oracle_mod, first_shape):
    """Over an estimate of 8 items the launches have fewer workgroups than over the library's estimate, crew included, and
    gather exactly the same surface points: the crew's workgroups evaluated what the regular ones did not."""
    prob, ref, prof = first_shape
    got, prof8 = solve(capi, oracle_mod, prob, {"GTO_ITEM_HINT": "8"}, profile=True, max_iter=MAX_ITER)
    assert_same(ref, got)
    print("reference:", prof[K_OBS], prof[K_STEP], "| hint 8:", prof8[K_OBS], prof8[K_STEP])
    assert prof[K_STEP][1] > 10 and prof8[K_STEP][1] > 10, (prof, prof8)  # the step kernel that writes the item lists ran
    assert prof8[K_OBS][1] == prof[K_OBS][1], (prof8[K_OBS], prof[K_OBS])  # one evaluation launch per round either way
    assert prof8[K_OBS][2] < prof[K_OBS][2], (prof8[K_OBS], prof[K_OBS])   # workgroups
    assert prof8[K_OBS][3] == prof[K_OBS][3] and prof[K_OBS][3] > 0, (prof8[K_OBS], prof[K_OBS])  # points gathered


@pytest.mark.parametrize("hint", [8, None])
def test_lanes_of_one_call(capi, oracle_mod, first_shape, hint):
    """Two lanes of 80 instances, each with item lists and launches of its own: the one-lane call's bits."""
    prob, ref, _ = first_shape
    got, _ = solve(capi, oracle_mod, prob, {} if hint is None else {"GTO_ITEM_HINT": str(hint)}, lanes=(2, 64, 0), max_iter=MAX_ITER)
    assert_same(ref, got)


def test_short_horizon_one_group_per_job(capi, oracle_mod):
    """Five waypoints: a job is ONE waypoint group, so an item is a job and the list is at its shortest against the crew."""
    T = 5
    prob = Problem("panda", B=130, scene_seed=4, n=64, res=0.035, n_goals=1, T=T)
    kw = dict(max_iter=30, T=T, standoff_offset=-1)
    plain, _ = solve(capi, oracle_mod, prob, {}, **kw)
    hinted, _ = solve(capi, oracle_mod, prob, {"GTO_ITEM_HINT": "8"}, **kw)
    off, _ = solve(capi, oracle_mod, prob, {"GTO_PREBROAD": "0"}, **kw)
    assert_same(plain, hinted)
    assert_same(plain, off)
