"""GPU: round 0 itemized from the seed test (GTO_SEED_PB_ALL).

In a lane with more instances than slots k_seed_broad tests the seeds that wait for a slot.  With GTO_SEED_PB_ALL (default on)
a second launch of it tests the seeds that START in a slot as well: it writes the records of the groups it settles into
set 1 and puts the others on round 0's item list, and the host plans round 0 as an itemized launch like every full round
behind it -- over the previous call's items per job when the handle has solved before, over the upper bound otherwise, with
the crew behind a short estimate.  A settled group contributes exact zeros, so every output of a call is the same bits as
with GTO_SEED_PB_ALL=0, where round 0 starts a workgroup for every group of every seed: assert_array_equal throughout.

Modelled on test_gpu_seed_broad_phase.py (its conventions: a fresh handle under the environment of the case, a few slots,
GTO_FEW_INSTANCES low so that they count as a full round): 24 instances on eight slots, sixteen refills."""
import numpy as np
import pytest

import test_gpu_broad_phase_verify as verify
import test_gpu_culling as culling
import test_gpu_seed_broad_phase as sbp
from helpers import Problem
from test_gpu_seed_broad_phase import debug_library  # noqa: F401  (the -DGTO_DEBUG_LONGEST_WG build, shared within a session)

pytestmark = pytest.mark.gpu

K_OBS, K_STEP = sbp.K_OBS, sbp.K_STEP
KNOBS = sbp.KNOBS + ("GTO_SEED_PB_ALL",)
SMALL = sbp.SMALL
ALL_OFF = {"GTO_SEED_PB_ALL": "0"}
MAX_ITER = 30
HORIZONS = {10: -2, 50: -10}  # T -> standoff_offset


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


def run(make_handle, args, env, calls=1):
    """`calls` solves of the same arguments on ONE fresh handle under env: the last call's outputs and profiles."""
    with pytest.MonkeyPatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        h = make_handle()
        h.set_profiling(True)
        a = args() if callable(args) else args
        outs = [h.solve_batch(*a) for _ in range(calls)]
        r = sbp.Run(outs[-1], h.last_kernel_profile(), h.last_seed_test_profile())
        r.first = outs[0]
        h.close()
    return r


def problem(robot, T):
    if robot == "fetch":  # the shelf
        return Problem("fetch", B=24, scene_seed=5, n=64, res=0.035, n_goals=1, T=T, shelf=True, table_z=0.75)
    return Problem("panda", B=24, scene_seed=5, n=64, res=0.035, n_goals=1, T=T)


def pair(capi, oracle_mod, prob, env, args=None, calls=1):
    """(default, GTO_SEED_PB_ALL=0) of one problem under env."""
    def make():
        h = capi.SolverHandle(prob.desc, prob.cfg["link_ee"], prob.cfg["link_gripper"],
                              oracle_mod.reference_opts(T=prob.T, standoff_offset=HORIZONS[prob.T], max_iter=MAX_ITER), device=0)
        h.set_mode(0)
        if getattr(prob, "goals", None) is None:
            prob.finish(h.eval_fk)
        h.set_scene(*prob.scene_args())
        return h
    return [run(make, prob.solve_args if args is None else args, dict(env, **e), calls) for e in ({}, ALL_OFF)]


def check_pair(on, off, waiting=16):
    """The same bits; the seed kernel's profiled launch is the waiting seeds' in both; full rounds ran (how many the host
    enqueues past the last instance's end depends on when it sees the end: not compared); round 0's list is a subset of
    its groups, so the obstacle launches gather no more points than with a plain round 0."""
    sbp.assert_same(on, off)
    assert on.seed[1:] == (1, waiting) and off.seed[1:] == (1, waiting), (on.seed, off.seed)
    assert on.prof[K_STEP][1] > 3 and off.prof[K_STEP][1] > 3, (on.prof, off.prof)
    assert 0 < on.prof[K_OBS][3] <= off.prof[K_OBS][3], (on.prof, off.prof)


def per_launch(r):
    """Workgroups per full-round obstacle launch.  The slots keep their positions, so every full round of a call has the same
    jobs and, under a fixed estimate or none, the same grid -- except a plain round 0, which is laid out over every group;
    the mean does not depend on how many rounds the host enqueued past the last instance's end."""
    return r.prof[K_OBS][2] / r.prof[K_OBS][1]


@pytest.mark.parametrize("robot,T", [("panda", 10), ("panda", 50), ("fetch", 10), ("fetch", 50)])
def test_round_0_itemized_keeps_every_bit(capi, oracle_mod, robot, T):
    """A fresh handle has no estimate: round 0's launch is laid out over the upper bound, as many workgroups as the plain one."""
    on, off = pair(capi, oracle_mod, problem(robot, T), SMALL)
    print(robot, T, "on:", on.prof[K_OBS], "| off:", off.prof[K_OBS])
    check_pair(on, off)
    assert per_launch(on) <= per_launch(off), (on.prof[K_OBS], off.prof[K_OBS])


# a launch gets a crew when the estimate plus the crew's 64 workgroups is short of its upper bound: 128 workgroups for
# eight slots of sixteen groups (T = 50); at T = 10 twelve slots (a grid for sixteen) of eight one-waypoint groups
CREW_ENV = {50: (SMALL, 16), 10: ({"GTO_SLOTS": "12", "GTO_FEW_INSTANCES": "4", "GTO_OBS_TG": "1"}, 12)}


@pytest.mark.parametrize("robot,T", [("panda", 10), ("panda", 50), ("fetch", 50)])
def test_short_estimate_leaves_round_0_to_the_crew(capi, oracle_mod, robot, T):
    """GTO_ITEM_HINT=8: eight regular workgroups per itemized launch, the crew at the end of the grid walks the rest of the
    list -- round 0's among them, which therefore starts fewer workgroups than the plain round 0 does."""
    prob = problem(robot, T)
    env, waiting = CREW_ENV[T]
    on, off = pair(capi, oracle_mod, prob, dict(env, GTO_ITEM_HINT="8"))
    print(robot, T, "on:", on.prof[K_OBS], "| off:", off.prof[K_OBS])
    check_pair(on, off, waiting)
    assert per_launch(on) < per_launch(off), (on.prof[K_OBS], off.prof[K_OBS])
    ref, _ = pair(capi, oracle_mod, prob, env)
    sbp.assert_same(ref, on)


def test_seeds_that_settle_every_group_leave_round_0_empty(capi, oracle_mod):
    """The far family of test_gpu_culling.py with every instance 5 m (beyond the distance field's cap) from the only non-zero
    voxels: every seed settles whole, round 0's list is empty and so is every list behind it -- no point is gathered in the
    whole call, and the host lays launches out over a published length of zero."""
    st = culling.Setup(oracle_mod, "panda", B=24, T=20, off=-4, seed=7, base=culling.FAR_BASE)
    fb = culling.contributing_fields(st, "far", seed=3)[0]
    st.base[:, 0] -= 5.0

    def make():
        h = st.handle(capi, oracle_mod, max_iter=25)
        h.set_scene(*fb.scene_args())
        return h
    on, off = [run(make, st.solve_args(), dict(SMALL, **e)) for e in ({}, ALL_OFF)]
    sbp.assert_same(on, off)
    assert on.seed[1:] == (1, 16), on.seed
    assert on.prof[K_OBS][3] == 0 and off.prof[K_OBS][3] == 0, (on.prof[K_OBS], off.prof[K_OBS])
    assert per_launch(on) <= per_launch(off), (on.prof[K_OBS], off.prof[K_OBS])


def test_seed_in_a_slot_with_a_nan(capi, oracle_mod):
    """A NaN in an optimised joint of the seed of instance 3, which starts in a slot: the seed kernel lists every group of it
    and writes no record, the obstacle kernel evaluates it whole, and it ends in GTO_STATUS_NUMERICAL with 0 iterations as
    in test_gpu_parity.py; the others keep the bits of the clean call."""
    prob = problem("panda", 10)
    clean, _ = pair(capi, oracle_mod, prob, SMALL)
    Q0 = prob.Q0.copy()
    Q0[3, prob.desc.opt_index[1], prob.T // 2] = np.nan
    on, off = pair(capi, oracle_mod, prob, SMALL, args=lambda: prob.solve_args()[:6] + (Q0,))
    sbp.assert_same(on, off)
    assert on.out[4][3] == capi.GTO_STATUS_NUMERICAL and on.out[3][3] == 0, (on.out[4].tolist(), on.out[3].tolist())
    others = np.setdiff1d(np.arange(prob.B), [3])
    assert (on.out[4][others] != capi.GTO_STATUS_NUMERICAL).all()
    for a, b in zip(clean.out, on.out):
        np.testing.assert_array_equal(a[others], b[others])


# (the estimate from the prior is 1.25 x items per job x jobs + 256: short of the upper bound only where that is large,
# twenty slots of forty-eight one-waypoint groups at T = 50)
PRIOR_ENV = {10: (SMALL, 16), 50: ({"GTO_SLOTS": "20", "GTO_FEW_INSTANCES": "4", "GTO_OBS_TG": "1"}, 4)}


@pytest.mark.parametrize("T", [10, 50])
def test_second_call_lays_round_0_out_over_the_prior(capi, oracle_mod, T):
    """The second call on a handle has the first one's items per job: its round 0 is laid out over that estimate, with the
    crew behind it where the estimate is short of the upper bound, and both calls give the bits of the plain ones.  (The
    workgroup totals are printed, not compared: the later rounds' estimates depend on which round the host saw last.)"""
    env, waiting = PRIOR_ENV[T]
    on, off = pair(capi, oracle_mod, problem("panda", T), env, calls=2)
    print(T, "second call on:", on.prof[K_OBS], "| off:", off.prof[K_OBS])
    check_pair(on, off, waiting)
    for a, b in zip(on.first, on.out):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(on.first, off.first):
        np.testing.assert_array_equal(a, b)


def test_settled_groups_of_round_0_get_no_contribution(debug_library, tmp_path):  # noqa: F811
    """test_gpu_seed_broad_phase.py's check on the debug build (GTO_DEBUG_CUT=10: every group listed, the settled ones marked):
    40 instances on eight slots.  With the seeds in slots tested, round 0's settled groups are marked too -- more marked groups
    than with GTO_SEED_PB_ALL=0, none of them with a contribution, the same results as the shipped library's."""
    env = {"GTO_HIP_LIB": debug_library, "GTO_DEBUG_TIMING": "1", "GTO_DEBUG_CUT": "10", "GTO_SLOTS": "8", "GTO_FEW_INSTANCES": "4"}
    a, b, c = (str(tmp_path / n) for n in ("all.npz", "waiting.npz", "plain.npz"))
    settled_on, contrib_on = sbp._settled(verify._run("panda_5k", 40, a, env))
    settled_off, contrib_off = sbp._settled(verify._run("panda_5k", 40, b, dict(env, GTO_SEED_PB_ALL="0")))
    print("settled groups with / without the seeds in slots:", settled_on, settled_off)
    assert contrib_on == 0 and contrib_off == 0
    assert settled_on > settled_off > 0
    verify._run("panda_5k", 40, c, {"GTO_SLOTS": "8", "GTO_FEW_INSTANCES": "4"})  # the shipped library
    va, vb, vc = np.load(a), np.load(b), np.load(c)
    for k in ("Q", "f", "it", "st"):
        np.testing.assert_array_equal(va[k], vb[k])
        np.testing.assert_array_equal(va[k], vc[k])
