"""GPU: the broad phase of the seeds that wait for a slot (k_seed_broad).

A call with more instances than slots starts the waiting ones as others finish: the finishing step workgroup hands its slot
to the next instance and puts the groups of that instance's SEED on the next round's item list.  k_seed_broad tests every
waiting seed once, behind the init pass, with the step kernel's own test (pb_test: the tail's tables, radius and groups), writes
the records of the groups it settles and leaves a bit mask of the others; the hand-over then lists the mask's groups instead
of all of them.  A settled group contributes exact zeros, so every output of a call is the same bits with the kernel
(default), without it (GTO_SEED_PB=0) and without any broad phase in the step kernel (GTO_PREBROAD=0); assert_array_equal
throughout, and one case against the oracle at the tolerances of test_gpu_parity.py.

Conventions of test_gpu_crew_fold.py: the library reads its knobs when a handle is created and when a call starts, so both
happen under the environment of the case; GTO_FEW_INSTANCES is set low so that a handful of slots count as a full round."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import small_robots as sr
import test_gpu_broad_phase_verify as verify
import test_gpu_culling as culling
from helpers import Problem

pytestmark = pytest.mark.gpu

K_OBS, K_STEP = "k_obstacle_gram<8,1>", "k_lm_step<4,1>"
KNOBS = ("GTO_ITEM_HINT", "GTO_SLOTS", "GTO_PREBROAD", "GTO_ITEM_GRID", "GTO_SEED_PB", "GTO_FEW_INSTANCES", "GTO_AHEAD", "GTO_OBS_TG")
OFF = ({"GTO_SEED_PB": "0"}, {"GTO_PREBROAD": "0"})  # the two calls every case is compared with
SMALL = {"GTO_SLOTS": "8", "GTO_FEW_INSTANCES": "4"}  # eight slots, and eight in flight are a full round
MAX_ITER = 30


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


class Run:
    """One call on a fresh handle: outputs, the solve loop's kernel profile, (ms, launches, workgroups) of k_seed_broad."""

    def __init__(self, out, prof, seed_prof):
        self.out, self.prof, self.seed = out, prof, seed_prof


def run(make_handle, args, env, lanes=None):
    """make_handle() -> a handle with its scene set; created, and the call made, under env.  args: the call's arguments, or a
    function that returns them once the handle exists (helpers.Problem draws its goals from the handle's kinematics)."""
    with pytest.MonkeyPatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        h = make_handle()
        if lanes is not None:
            h.set_lanes(*lanes)
        h.set_profiling(True)
        out = h.solve_batch(*(args() if callable(args) else args))
        r = Run(out, h.last_kernel_profile(), h.last_seed_test_profile())
        h.close()
    for a in r.out:
        a.setflags(write=False)
    return r


def assert_same(ref, got):
    for a, b in zip(ref.out, got.out):  # Q, dQ, cost, iterations, status
        np.testing.assert_array_equal(a, b)


def problem_runs(capi, oracle_mod, prob, env, lanes=None, args=None, **opt_kw):
    """(default, GTO_SEED_PB=0, GTO_PREBROAD=0) of one problem under env."""
    def make():
        h = capi.SolverHandle(prob.desc, prob.cfg["link_ee"], prob.cfg["link_gripper"], oracle_mod.reference_opts(**opt_kw), device=0)
        h.set_mode(0)
        if getattr(prob, "goals", None) is None:
            prob.finish(h.eval_fk)
        h.set_scene(*prob.scene_args())
        return h

    def go(e):
        return run(make, prob.solve_args if args is None else args, dict(env, **e), lanes)
    return go({}), go(OFF[0]), go(OFF[1])


def check_three(on, off, plain, waiting, launches=1):
    """The three calls give the same bits; the seed kernel ran once per lane with waiting instances, one workgroup per
    waiting instance, and only in the default call; the step kernel that lists the items ran."""
    assert_same(on, off)
    assert_same(on, plain)
    assert on.seed[1:] == (launches, waiting), on.seed
    assert off.seed[1:] == (0, 0) and plain.seed[1:] == (0, 0), (off.seed, plain.seed)
    assert on.prof[K_STEP][1] > 3 and off.prof[K_STEP][1] == on.prof[K_STEP][1], (on.prof, off.prof)
    # points gathered: the masks' items are a subset of all items (a settled group may hold a chunk whose own sphere
    # survives the obstacle kernel's per-chunk test and gathers exact zeros: DESIGN.md section 5)
    assert 0 < on.prof[K_OBS][3] <= off.prof[K_OBS][3], (on.prof, off.prof)


@pytest.fixture(scope="module")
def refills(capi, oracle_mod):
    """Panda, 24 instances on eight slots, T = 50: sixteen refills, sixteen groups of three waypoints each."""
    prob = Problem("panda", B=24, scene_seed=5, n=64, res=0.035, n_goals=1)
    return (prob,) + problem_runs(capi, oracle_mod, prob, SMALL, max_iter=MAX_ITER)


def test_refills_keep_every_bit(refills):
    prob, on, off, plain = refills
    check_three(on, off, plain, waiting=16)


def test_refills_match_oracle(oracle_mod, refills):
    prob, on, _, _ = refills
    o = oracle_mod.Oracle(prob.desc, prob.cfg["link_ee"], prob.cfg["link_gripper"], oracle_mod.reference_opts(max_iter=MAX_ITER))
    o.set_scene(*prob.scene_args())
    Qo, dQo, fo, ito, sto = o.solve_batch(*prob.solve_args())
    np.testing.assert_array_equal(on.out[3], ito)  # the refills (instances 8 .. 23) included
    np.testing.assert_array_equal(on.out[4], sto)
    np.testing.assert_allclose(on.out[0], Qo, rtol=0, atol=1e-6)


def test_shortest_horizon_has_no_room_for_the_test(capi, oracle_mod):
    """T = 5, one group of three waypoints per job: the Panda's tables do not fit the step kernel's LDS at this horizon
    (PbLayout: no waypoint per pass), so neither the tail nor the seed kernel runs; the three calls are the same call."""
    T = 5
    prob = Problem("panda", B=24, scene_seed=4, n=64, res=0.035, n_goals=1, T=T)
    on, off, plain = problem_runs(capi, oracle_mod, prob, SMALL, max_iter=MAX_ITER, T=T, standoff_offset=-1)
    assert_same(on, off)
    assert_same(on, plain)
    assert on.seed[1:] == (0, 0), on.seed


def test_one_group_per_job(capi, oracle_mod):
    """One group per job where the test has room: T = 10 with groups of eight waypoints (GTO_OBS_TG=8).  A seed's mask is one
    bit, and a refill lists one item or none."""
    T = 10
    prob = Problem("panda", B=24, scene_seed=4, n=64, res=0.035, n_goals=1, T=T)
    on, off, plain = problem_runs(capi, oracle_mod, prob, dict(SMALL, GTO_OBS_TG="8"), max_iter=MAX_ITER, T=T, standoff_offset=-2)
    check_three(on, off, plain, waiting=16)


def test_smallest_refill(capi, oracle_mod):
    """Five slots for seven instances: two waiting seeds, one refill at a time."""
    prob = Problem("panda", B=7, scene_seed=5, n=64, res=0.035, n_goals=1)
    on, off, plain = problem_runs(capi, oracle_mod, prob, {"GTO_SLOTS": "5", "GTO_FEW_INSTANCES": "4"}, max_iter=MAX_ITER)
    check_three(on, off, plain, waiting=2)


def test_short_estimate_leaves_masked_items_to_the_crew(capi, oracle_mod, refills):
    """An estimate of eight items for launches of up to 128: the crew at the end of the grid evaluates what the masks list."""
    prob, ref, _, _ = refills
    on, off, plain = problem_runs(capi, oracle_mod, prob, dict(SMALL, GTO_ITEM_HINT="8"), max_iter=MAX_ITER)
    check_three(on, off, plain, waiting=16)
    assert_same(ref, on)
    assert on.prof[K_OBS][2] < ref.prof[K_OBS][2], (on.prof[K_OBS], ref.prof[K_OBS])  # the estimate was in force


def test_two_lanes(capi, oracle_mod):
    """Two lanes of sixteen instances on eight slots each: a launch of the seed kernel per lane, eight waiting seeds each;
    the masks are indexed by instance, whichever lane's lists it is on."""
    prob = Problem("panda", B=32, scene_seed=5, n=64, res=0.035, n_goals=1)
    on, off, plain = problem_runs(capi, oracle_mod, prob, SMALL, lanes=(2, 8, 0), max_iter=MAX_ITER)
    assert_same(on, off)
    assert_same(on, plain)
    assert on.seed[1:] == (2, 16) and off.seed[1:] == (0, 0), (on.seed, off.seed)
    one_lane, _, _ = problem_runs(capi, oracle_mod, prob, SMALL, max_iter=MAX_ITER)
    assert_same(on, one_lane)


def test_waiting_seed_with_a_nan(capi, oracle_mod, refills):
    """A NaN in an optimised joint of a waiting seed (instance 13 of 24 on eight slots): the seed kernel leaves that seed to
    the obstacle kernel whole (full mask, no record), it ends in GTO_STATUS_NUMERICAL with 0 iterations as in
    test_gpu_parity.py, and every other instance keeps the bits of the clean call."""
    prob, clean, _, _ = refills
    Q0 = prob.Q0.copy()
    Q0[13, prob.desc.opt_index[1], prob.T // 2] = np.nan
    args = lambda: prob.solve_args()[:6] + (Q0,)
    on, off, plain = problem_runs(capi, oracle_mod, prob, SMALL, args=args, max_iter=MAX_ITER)
    check_three(on, off, plain, waiting=16)
    assert on.out[4][13] == capi.GTO_STATUS_NUMERICAL and on.out[3][13] == 0, (on.out[4].tolist(), on.out[3].tolist())
    others = np.setdiff1d(np.arange(prob.B), [13])
    assert (on.out[4][others] != capi.GTO_STATUS_NUMERICAL).all()
    for a, b in zip(clean.out, on.out):
        np.testing.assert_array_equal(a[others], b[others])


def culling_runs(capi, oracle_mod, family, B, env, base=(0.0, 0.0, 0.0), apart=0.0):
    """The three calls on a field of one of test_gpu_culling.py's families (thin Panda, T = 20, designs at the seeds of
    instances 0 and 1); apart: instances 2 .. B - 1 stand that far down the x axis from the first two."""
    st = culling.Setup(oracle_mod, "panda", B=B, T=20, off=-4, seed=7, base=base)
    st.base[2:, 0] -= apart
    fb = culling.contributing_fields(st, family, seed=3)[0]

    def make():
        h = st.handle(capi, oracle_mod, max_iter=25)
        h.set_scene(*fb.scene_args())
        return h
    return [run(make, st.solve_args(), dict(env, **e)) for e in ({},) + OFF]


def test_seeds_in_free_space_cost_no_workgroup(capi, oracle_mod):
    """The far family (tests/cull_fields.py: a 30 m grid, the base shifted into it) with its only non-zero voxels next to
    instances 0 and 1 and every other instance 5 m (166 voxels, beyond the distance field's cap) down the grid: every waiting
    seed stands in free space, its mask is empty and its refill puts nothing on the item list.  384 instances on 128 slots, six
    groups each: the itemized launches are laid out over the estimate of their lists (floor 256, bound 768), which is lower
    without the refills' six items each than with them (GTO_AHEAD=1: the estimate is at most two rounds old); the points
    gathered -- by instances 0 and 1 -- are the same."""
    env = {"GTO_SLOTS": "128", "GTO_FEW_INSTANCES": "16", "GTO_AHEAD": "1"}
    on, off, plain = culling_runs(capi, oracle_mod, "far", 384, env, base=culling.FAR_BASE, apart=5.0)
    print("seed test on:", on.prof[K_OBS], on.seed, "| off:", off.prof[K_OBS])
    check_three(on, off, plain, waiting=256)
    assert on.prof[K_OBS][1] == off.prof[K_OBS][1], (on.prof[K_OBS], off.prof[K_OBS])  # launches
    assert on.prof[K_OBS][2] < off.prof[K_OBS][2], (on.prof[K_OBS], off.prof[K_OBS])   # workgroups
    assert on.prof[K_OBS][3] == off.prof[K_OBS][3], (on.prof[K_OBS], off.prof[K_OBS])  # points gathered


def test_seeds_that_touch_the_band_everywhere(capi, oracle_mod):
    """The edge family on its coarse grid (every sphere of every group within its culling radius of a non-zero record): full
    masks, the hand-over lists what it always listed, the launches have the same workgroups and gather the same points."""
    on, off, plain = culling_runs(capi, oracle_mod, "edge", 24, SMALL)
    print("seed test on:", on.prof[K_OBS], on.seed, "| off:", off.prof[K_OBS])
    check_three(on, off, plain, waiting=16)
    assert on.prof[K_OBS][1:] == off.prof[K_OBS][1:], (on.prof[K_OBS], off.prof[K_OBS])  # launches, workgroups, points gathered


def test_wide_robot_never_launches_the_seed_kernel(capi, oracle_mod):
    """Nine optimised joints (tests/small_robots.py, chain_9_short): the 16-wide kernels have no broad phase in the step
    kernel, so four instances on two slots refill as they always did, and k_seed_broad is not launched."""
    case = sr.Case(oracle_mod, "chain_9_short", 5)
    env = {"GTO_SLOTS": "2", "GTO_FEW_INSTANCES": "1"}
    on, off = (run(lambda: case.handle(capi), case.solve_args(), dict(env, **e)) for e in ({}, OFF[0]))
    assert_same(on, off)
    assert on.seed[1:] == (0, 0) and off.seed[1:] == (0, 0), (on.seed, off.seed)
    assert on.prof["k_lm_step_wide<16>"][1] > 3, on.prof  # full rounds of the wide step kernel, refills among them


# ------------------------------------------------------------------------------------------ the debug build's verification
@pytest.fixture(scope="module")
def debug_library(tmp_path_factory):
    """The -DGTO_DEBUG_LONGEST_WG build of test_gpu_broad_phase_verify.py: the one that module built in this session, if it ran."""
    built = glob.glob(os.path.join(str(tmp_path_factory.getbasetemp()), "dbg*", "libgto_hip_dbg.so"))
    if built:
        return built[0]
    lib = str(tmp_path_factory.mktemp("dbg") / "libgto_hip_dbg.so")
    sys.path.insert(0, verify.ROOT)
    import __graft_entry__ as g
    src = [os.path.join(g.CSRC, s) for s in g.HIP_SOURCES]
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + g.HIPCC_FLAGS + ["-DGTO_DEBUG_LONGEST_WG"] + src + ["-o", lib],
                          cwd=g.CSRC, stderr=subprocess.DEVNULL)
    return lib


def _settled(err):
    lines = [l for l in err.splitlines() if "groups settled" in l]
    assert lines, err[-2000:]
    m = re.search(r"(\d+) groups settled, (\d+) of them with a surviving chunk, (\d+) with a CONTRIBUTION", lines[-1])
    assert m, lines[-1]
    return int(m.group(1)), int(m.group(3))


def test_settled_groups_of_seeds_get_no_contribution(debug_library, tmp_path):
    """test_gpu_broad_phase_verify.py's check with refills in the call (its shapes have none: 512 and 320 instances fit the
    slots): 40 instances on eight slots, every group listed (GTO_DEBUG_CUT=10), the groups the seed kernel settled marked like
    the tail's -- more marked groups than without the seed kernel, none of them with a contribution, the same results."""
    env = {"GTO_HIP_LIB": debug_library, "GTO_DEBUG_TIMING": "1", "GTO_DEBUG_CUT": "10", "GTO_SLOTS": "8", "GTO_FEW_INSTANCES": "4"}
    a, b, c = (str(tmp_path / n) for n in ("seed.npz", "noseed.npz", "plain.npz"))
    settled_on, contrib_on = _settled(verify._run("panda_5k", 40, a, env))
    settled_off, contrib_off = _settled(verify._run("panda_5k", 40, b, dict(env, GTO_SEED_PB="0")))
    print("settled groups with / without the seed kernel:", settled_on, settled_off)
    assert contrib_on == 0 and contrib_off == 0
    assert settled_on > settled_off > 0
    verify._run("panda_5k", 40, c, {"GTO_SLOTS": "8", "GTO_FEW_INSTANCES": "4"})  # the shipped library
    va, vb, vc = np.load(a), np.load(b), np.load(c)
    for k in ("Q", "f", "it", "st"):
        np.testing.assert_array_equal(va[k], vb[k])
        np.testing.assert_array_equal(va[k], vc[k])
