"""GPU: the step kernels read their arguments from the kernel-argument segment, phase by phase (gto_kernels.h,
StepKernArgs), instead of holding them in scalar registers from the kernel's entry.  What that can break is an argument or a
per-instance uniform read from the wrong place on a path the large workloads rarely take: the shortest horizons, the exits
through GTO_FINISH, slots handed over mid-call with the tail's broad phase, static list positions and seed masks on, a robot
with actuated joints that are not optimised (the tail's s_qp and header), a non-finite seed among the waiting instances.

Every case is compared with the FP64 oracle as tests/test_gpu_parity.py compares: iteration counts and status equal,
trajectories within 1e-6 rad after the same number of iterations, objectives to 1e-7 relative.  No call has more than 24
instances."""
import numpy as np
import pytest

import small_robots as sr
from helpers import Problem

pytestmark = pytest.mark.gpu

Q_ATOL, F_RTOL = 1e-6, 1e-7   # tests/test_gpu_parity.py: solved trajectories after the same number of iterations; objectives


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


def _pair(capi, oracle_mod, monkeypatch, prob, env, **opt_kw):
    """A handle created under `env` (the library reads its tunables when a handle is made) and the oracle of the same problem."""
    opts = oracle_mod.reference_opts(**opt_kw)
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        h = capi.SolverHandle(prob.desc, prob.cfg["link_ee"], prob.cfg["link_gripper"], opts, device=0)
    h.set_mode(0)
    o = oracle_mod.Oracle(prob.desc, prob.cfg["link_ee"], prob.cfg["link_gripper"], opts)
    prob.finish(h.eval_fk)
    h.set_scene(*prob.scene_args())
    o.set_scene(*prob.scene_args())
    return h, o


def _check(got, ref, what):
    Qg, _, fg, itg, stg = got
    Qo, _, fo, ito, sto = ref
    print(f"{what}: iterations gpu {itg.tolist()} oracle {ito.tolist()} status {stg.tolist()} max |Q - Q_oracle| {np.abs(Qg - Qo).max():.3e}")
    np.testing.assert_array_equal(itg, ito)
    np.testing.assert_array_equal(stg, sto)
    np.testing.assert_allclose(Qg, Qo, rtol=0, atol=Q_ATOL)
    np.testing.assert_allclose(fg, fo, rtol=F_RTOL)


# T = 14 / 15: the boundary from which the tail's tables fit behind the trial point (pb_table_doubles); T = 4: the smallest horizon
@pytest.mark.parametrize("max_iter", [1, 2, 60])  # GTO_FINISH at the iteration cap after one and two evaluations; a solve that converges
@pytest.mark.parametrize("T", [4, 14, 15])
@pytest.mark.parametrize("B", [1, 3])
def test_few_instances_short_horizons(capi, oracle_mod, monkeypatch, B, T, max_iter):
    """k_lm_step<8,4>: four candidates per step, on the Panda with 1 200 surface points."""
    prob = Problem("panda", B=B, scene_seed=3, T=T)
    kw = dict(max_iter=max_iter, T=T, standoff_offset=-1 if T == 4 else -3)
    h, o = _pair(capi, oracle_mod, monkeypatch, prob, {}, **kw)
    h.set_profiling(True)
    got = h.solve_batch(*prob.solve_args())
    prof = h.last_kernel_profile()
    assert prof["k_lm_step<8,4>"][1] >= 1 and prof["k_lm_step<4,1>"][1] == 0, prof
    ref = o.solve_batch(*prob.solve_args())
    _check(got, ref, f"B={B} T={T} max_iter={max_iter}")
    if max_iter <= 2:
        assert (got[3] <= max_iter).all()
    else:
        assert (got[4] == capi.GTO_STATUS_CONVERGED).any(), got[4].tolist()
    h.close()


REFILL = [("panda", 15, {}), ("panda", 50, {}), ("fetch", 15, {}), ("fetch", 50, {}),
          ("panda", 15, {"GTO_FEW_INSTANCES": "2"}), ("panda", 50, {"GTO_FEW_INSTANCES": "2"}),
          ("fetch", 15, {"GTO_FEW_INSTANCES": "2"}), ("fetch", 50, {"GTO_FEW_INSTANCES": "2"}),
          ("fetch", 15, {"GTO_FEW_INSTANCES": "2", "GTO_PREBROAD": "0"}), ("panda", 50, {"GTO_FEW_INSTANCES": "2", "GTO_STATIC_POS": "0"})]


@pytest.mark.parametrize("robot,T,env", REFILL, ids=[f"{r}-T{T}-" + ("+".join(f"{k[4:]}={v}" for k, v in e.items()) or "few") for r, T, e in REFILL])
def test_refills_through_few_slots(capi, oracle_mod, monkeypatch, robot, T, env):
    """24 instances through 8 slots: an instance that finishes hands its slot to one that waits (GTO_FINISH: the newcomer's
    joint values, its seed mask, its list entries).  As shipped the rounds run k_lm_step<8,4>; with GTO_FEW_INSTANCES=2 they run
    k_lm_step<4,1> with its tail, static positions and the seed masks until two instances are left.  The Fetch has eight
    actuated joints that are not optimised: the tail reads their values (s_qp) and a header of another size."""
    prob = Problem(robot, B=24, scene_seed=2, T=T, n_goals=2 if robot == "panda" else 1)
    kw = dict(max_iter=12, T=T, standoff_offset=-max(2, T // 5))
    h, o = _pair(capi, oracle_mod, monkeypatch, prob, dict(env, GTO_SLOTS="8"), **kw)
    h.set_profiling(True)
    got = h.solve_batch(*prob.solve_args())
    prof = h.last_kernel_profile()
    if "GTO_FEW_INSTANCES" in env:
        assert prof["k_lm_step<4,1>"][1] > 5, prof  # the variant under test ran
    else:
        assert prof["k_lm_step<8,4>"][1] > 5, prof
    h.set_profiling(False)
    again = h.solve_batch(*prob.solve_args())  # the second call reuses the workspace and the lists of the first
    for a, b in zip(got, again):
        np.testing.assert_array_equal(a, b)
    ref = o.solve_batch(*prob.solve_args())
    _check(got, ref, f"{robot} T={T} {env}")
    assert len(set(ref[3].tolist())) > 1  # instances finish at different rounds: slots are handed over mid-solve
    h.close()


def test_smallest_robot_at_its_smallest_size(capi, oracle_mod, monkeypatch):
    """tests/small_robots.py: one joint, T = 4, a 5 x 5 x 5 field; through the launches for few instances and, with
    GTO_FEW_INSTANCES=0, through the one-candidate kernel and its tail."""
    c = sr.Case(oracle_mod, "chain_1", 4)
    o = c.oracle(oracle_mod)
    ref = o.solve_batch(*c.solve_args())
    for env in ({}, {"GTO_FEW_INSTANCES": "0"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            h = c.handle(capi)
        _check(h.solve_batch(*c.solve_args()), ref, f"chain_1 T=4 {env}")
        h.close()


@pytest.mark.parametrize("env", [{}, {"GTO_FEW_INSTANCES": "2"}], ids=["few", "FEW_INSTANCES=2"])
def test_non_finite_seed_through_the_refill_path(capi, oracle_mod, monkeypatch, env):
    """A NaN in the seed of an instance that WAITS for a slot (12 instances, 4 slots: instance 9 starts in a slot an earlier
    one hands over): it ends in GTO_STATUS_NUMERICAL with 0 iterations, as in the oracle, hands the slot on in the same
    launch, and every other instance gets the bits it gets in the call without the poisoned seed."""
    B, T = 12, 15
    prob = Problem("panda", B=B, scene_seed=3, T=T, n_goals=1)
    kw = dict(max_iter=12, T=T, standoff_offset=-3)
    h, o = _pair(capi, oracle_mod, monkeypatch, prob, dict(env, GTO_SLOTS="4"), **kw)
    clean = h.solve_batch(*prob.solve_args())
    Q0 = prob.Q0.copy()
    Q0[9, prob.desc.opt_index[1], T // 2] = np.nan
    args = list(prob.solve_args())
    args[6] = Q0
    got = h.solve_batch(*args)
    ref = o.solve_batch(*args)
    np.testing.assert_array_equal(got[3], ref[3])
    np.testing.assert_array_equal(got[4], ref[4])
    assert got[4][9] == capi.GTO_STATUS_NUMERICAL and got[3][9] == 0, (got[4].tolist(), got[3].tolist())
    ok = np.setdiff1d(np.arange(B), [9])
    assert (got[4][ok] != capi.GTO_STATUS_NUMERICAL).all()
    for a, b in zip(got, clean):
        np.testing.assert_array_equal(a[ok], b[ok])
    np.testing.assert_allclose(got[0][ok], ref[0][ok], rtol=0, atol=Q_ATOL)
    np.testing.assert_allclose(got[2][ok], ref[2][ok], rtol=F_RTOL)
    h.close()
