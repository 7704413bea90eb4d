"""GPU: the init pass once per run of equal start states (k_init_heads, k_ss_fixed_spread; GTO_INIT_DEDUP).

The init pass of a solve call leaves four numbers per instance (ss_fixed) that depend on the instance's scene, base and
joint values at the two pinned waypoints only.  With GTO_INIT_DEDUP (default on, for calls of more than GTO_INIT_DEDUP_MIN / 4
instances) only the first instance of a run of equal keys inside a block of 64 computes them and the others get a copy.  A
copy of the same computation is the same bits, so every output of a call -- Q, dQ, cost, iterations, status -- and the
evaluation entry points' read-back of ss_fixed (gto_eval_obstacle_normal_eq: the sum of c^2 of waypoints 0 and 1;
gto_eval_objective: all four numbers inside f_obs) are compared for equality with GTO_INIT_DEDUP=0.  rep[] itself is not
read back: the cases are built so that the rule of tests/test_init_heads_cpu.py gives the pattern each one is about (asserted
here on the restatement), and a wrong representative shows as a wrong ss_fixed.

Panda at T = 10, GTO_INIT_DEDUP_MIN=1 so that calls of a few instances take the path.  The library reads its knobs when a
handle is created, so each call gets a fresh handle under its environment (the conventions of test_gpu_seed_broad_phase.py)."""
import numpy as np
import pytest

import small_robots as sr
import test_init_heads_cpu as rule
from helpers import Problem

pytestmark = pytest.mark.gpu

KNOBS = ("GTO_INIT_DEDUP", "GTO_INIT_DEDUP_MIN", "GTO_SLOTS", "GTO_FEW_INSTANCES")
ON, OFF = {"GTO_INIT_DEDUP_MIN": "1"}, {"GTO_INIT_DEDUP": "0"}
T, OFFSET, MAX_ITER = 10, -2, 15


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


class Batch:
    """A Panda problem of B instances with one start state, for a case to edit (qc, base, Q0, sid) before it runs."""

    def __init__(self, capi, oracle_mod, B, scene_seed=5):
        self.capi, self.oracle_mod = capi, oracle_mod
        self.p = Problem("panda", B=B, scene_seed=scene_seed, n=64, res=0.035, n_goals=1, T=T)
        self.B, self.desc = B, self.p.desc
        h = self.handle({})
        self.p.finish(h.eval_fk)
        h.close()
        self.qc, self.base, self.Q0 = self.p.qc.copy(), self.p.base.copy(), self.p.Q0.copy()
        self.sid = np.zeros(B, dtype=np.int32)
        self.shared = False   # scene 1 borrows scene 0's fields
        self.lanes = None

    def handle(self, env):
        p = self.p
        with pytest.MonkeyPatch.context() as mp:
            for k in KNOBS:
                mp.delenv(k, raising=False)
            for k, v in env.items():
                mp.setenv(k, v)
            h = self.capi.SolverHandle(p.desc, p.cfg["link_ee"], p.cfg["link_gripper"],
                                       self.oracle_mod.reference_opts(T=T, standoff_offset=OFFSET, max_iter=MAX_ITER), device=0)
        h.set_scene(*p.scene_args())
        return h

    def rep(self):
        return rule.init_heads(rule.keys(self.sid, self.base, rule.start_rows(self.desc, self.qc, self.Q0)))

    def outputs(self, env):
        """(Q, dQ, cost, iterations, status, sum c^2 of waypoints 0 and 1 as the evaluation reads it back, f_obs) of one handle."""
        h = self.handle(env)
        if self.shared:
            h.share_scene(1, h, 0)
        if self.lanes:
            h.set_lanes(*self.lanes)
        p = self.p
        out = h.solve_batch(self.sid, self.qc, p.goals, p.n_goals, p.S, self.base, self.Q0)
        Qe = self.Q0.copy()
        Qe[:, self.desc.opt_index, :2] = self.qc[:, self.desc.opt_index, None]  # the evaluation takes Q as given: the solve's pinned rows
        ss = h.eval_obstacle_normal_eq(self.sid, self.base, Qe)[2][:, :2]
        fo = h.eval_objective(self.sid, p.goals, p.n_goals, p.S, self.base, Qe)[1]
        h.close()
        return out + (ss, fo)

    def check(self, want_rep=None):
        """Same bits with and without the dedup; returns the outputs with it."""
        if want_rep is not None:
            np.testing.assert_array_equal(self.rep(), want_rep)
        on, off = self.outputs(ON), self.outputs(OFF)
        for a, b in zip(on, off):
            np.testing.assert_array_equal(a, b)
        return on


@pytest.mark.parametrize("B", [1, 2, 65, 130])
def test_all_keys_equal(capi, oracle_mod, B):
    """One start state: one head per block of 64 (B = 65 and 130: a block of one and of two instances at the end)."""
    b = Batch(capi, oracle_mod, B)
    on = b.check((np.arange(B) // rule.BLOCK) * rule.BLOCK)
    assert (on[5] == on[5][0]).all(), on[5][:2]  # every instance has the first one's numbers


def test_equal_keys_that_are_not_neighbours(capi, oracle_mod):
    b = Batch(capi, oracle_mod, 3)
    b.qc[1, b.desc.opt_index[1]] += 0.2
    on = b.check([0, 1, 2])
    np.testing.assert_array_equal(on[5][0], on[5][2])


def test_one_bit_differences(capi, oracle_mod):
    """Instance 1 differs from 0 in the last bit of base_pos[2] only; instance 3 from 2 in the last bit of one joint value of
    waypoint 1 only (a finger: a joint that is not optimised takes its pinned rows from the seed)."""
    b = Batch(capi, oracle_mod, 6)
    b.base[:, 2] = 0.01
    b.base[1:, 2] = np.nextafter(0.01, 1.0)
    dq = int(b.desc.param_index[0])
    b.Q0[3:, dq, 1] = np.nextafter(b.Q0[3, dq, 1], 1.0)
    b.check([0, 1, 1, 3, 3, 3])


def test_two_scene_ids_one_shared_field(capi, oracle_mod):
    """Scene 1 borrows scene 0's fields (gto_share_scene): the numbers are the same, the keys are not."""
    b = Batch(capi, oracle_mod, 6)
    b.shared = True
    b.sid[:] = [0, 0, 1, 1, 0, 0]
    on = b.check([0, 0, 2, 2, 4, 4])
    assert (on[5] == on[5][0]).all()


def test_signed_zero(capi, oracle_mod):
    b = Batch(capi, oracle_mod, 4)
    b.base[:] = 0.0
    b.base[1, 0] = -0.0
    b.check([0, 1, 2, 2])


def test_nan_in_qc(capi, oracle_mod):
    """A NaN in qc of instance 1, between two equal neighbours: it is a key of its own, ends in GTO_STATUS_NUMERICAL as it
    always did, and its neighbours keep the bits of the call without it."""
    clean = Batch(capi, oracle_mod, 3).check([0, 0, 0])
    b = Batch(capi, oracle_mod, 3)
    b.qc[1, b.desc.opt_index[2]] = np.nan
    np.testing.assert_array_equal(b.rep(), [0, 1, 2])
    on, off = b.outputs(ON), b.outputs(OFF)
    for x, y in zip(on, off):
        np.testing.assert_array_equal(x, y)  # (NaNs in the same places)
    assert on[4][1] == capi.GTO_STATUS_NUMERICAL and on[4][0] != capi.GTO_STATUS_NUMERICAL and on[4][2] != capi.GTO_STATUS_NUMERICAL, on[4]
    for x, y in zip(clean[:5], on[:5]):
        np.testing.assert_array_equal(x[[0, 2]], y[[0, 2]])


def test_run_boundary_at_the_block_edge(capi, oracle_mod):
    """The start state changes at instance 63, the last of block 0: 63 is a head by its key, 64 by its place."""
    B = 130
    b = Batch(capi, oracle_mod, B)
    b.qc[rule.BLOCK - 1:, b.desc.opt_index[0]] += 0.1
    want = (np.arange(B) // rule.BLOCK) * rule.BLOCK
    want[rule.BLOCK - 1] = rule.BLOCK - 1
    on = b.check(want)
    assert (on[5][:rule.BLOCK - 1] == on[5][0]).all() and (on[5][rule.BLOCK - 1:] == on[5][rule.BLOCK - 1]).all()


def test_lanes_inside_a_call(capi, oracle_mod):
    """Two lanes of sixteen instances: the init pass and rep[] index the batch, whichever lane an instance is on."""
    b = Batch(capi, oracle_mod, 32)
    b.qc[20:, b.desc.opt_index[3]] -= 0.1
    b.lanes = (2, 8, 0)
    want = np.zeros(32, dtype=np.int32)
    want[20:] = 20
    on = b.check(want)
    b.lanes = None
    for x, y in zip(on, b.outputs(ON)):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("kind", ["root_joint", "one_point"])
def test_smallest_robots(capi, oracle_mod, kind):
    """One frame with the joint on the root (root_joint) and the one-point robot, T = 4, four instances of which 0, 1 and 3
    share a start state (0 and 1 as neighbours)."""
    case = sr.Case(oracle_mod, kind, 4)
    qc, base, Q0 = case.qc.copy(), case.base.copy(), case.Q0.copy()
    for i in (1, 3):
        qc[i], base[i], Q0[i, :, :2] = qc[0], base[0], Q0[0, :, :2]
    np.testing.assert_array_equal(rule.init_heads(rule.keys(0, base, rule.start_rows(case.desc, qc, Q0))), [0, 0, 2, 3])
    outs = []
    for env in (ON, OFF):
        with pytest.MonkeyPatch.context() as mp:
            for k in KNOBS:
                mp.delenv(k, raising=False)
            for k, v in env.items():
                mp.setenv(k, v)
            h = case.handle(capi)
        outs.append(h.solve_batch(0, qc, case.goals, case.n_goals, case.S, base, Q0) + (h.eval_obstacle_normal_eq(0, base, Q0)[2][:, :2],))
        h.close()
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)
