"""gto_solve_ik_pose_batch on the MI355X on every branch of ik_orient_goal_wave's pose arithmetic: the case table of
tests/ik_pose_cases.py (a gimbal robot; the four Shepperd pivots and their boundaries, pitch up to and on the clamp, yaw
and roll at the atan2 cuts, goal quaternions of either sign and any norm, an optimised joint beside the chain) against the
numpy restatement (tests/ik_pose_ref.py) on the oracle's frames.  A comparison is widened by the case's sensitivity
allowance (the restatement's own change when the oracle's frame is turned by the 1e-13 to which eval_fk is held to the
oracle) and by nothing else.  Run it as its siblings: timeout -k 10 600 pytest -x tests/test_gpu_ik_pose_cases.py."""
import numpy as np
import pytest

import ik_pose_cases as ipc
import ik_pose_ref as ref
from grasptrajopt_amd import synthetic as syn

pytestmark = pytest.mark.gpu
Q, RPY = ref.GTO_IK_GOAL_QUATERNION, ref.GTO_IK_GOAL_RPY
OK = [ref.GTO_STATUS_CONVERGED, ref.GTO_STATUS_MAX_ITER]


class Ctx:
    """One handle, the table, and each solve of the whole table run once (keyed by scene and iteration cap)."""

    def __init__(self, capi, oracle_mod):
        self.desc, self.o, self.opts, self.cases = ipc.table(oracle_mod)
        self.h = capi.SolverHandle(self.desc, ipc.EE, ipc.EE, self.opts, device=0)
        sc = syn.make_scene(3, n=48, res=0.0467)
        for s in (self.h, self.o):
            s.set_scene(0, sc.c_all, sc.c_obs, sc.shape, sc.origin, sc.res)
        self.q0 = np.stack([c.q0 for c in self.cases])
        self.qc = ipc.clipped(self.desc, self.q0)
        self.fe = self.desc.frame_index(ipc.EE)
        self.T = self.o.eval_fk(self.qc)[:, self.fe]
        self.idx = {k: [i for i, c in enumerate(self.cases) if c.kind == k] for k in (Q, RPY)}
        self._runs, self._refs = {}, {}

    def solve(self, ids, max_iter, scene=False):
        """(q, cost, iters, status) of the cases ids, in that order, one launch per kind."""
        out = [None] * len(ids)
        for k in (Q, RPY):
            sel = [n for n, i in enumerate(ids) if self.cases[i].kind == k]
            if not sel:
                continue
            g = np.stack([self.cases[ids[n]].goal for n in sel])
            q0 = self.q0[[ids[n] for n in sel]]
            res = self.h.solve_ik_pose_batch(k, 0 if scene else None, q0, g, np.zeros((len(sel), 3)) if scene else None, max_iter=max_iter)
            for m, n in enumerate(sel):
                out[n] = tuple(r[m] for r in res)
        return out

    def run(self, max_iter, scene=False):
        key = (max_iter, scene)
        if key not in self._runs:
            self._runs[key] = self.solve(list(range(len(self.cases))), max_iter, scene)
        return self._runs[key]

    def ref(self, i, max_iter):
        if (i, max_iter) not in self._refs:
            c = self.cases[i]
            self._refs[i, max_iter] = ref.solve(ipc.problem(self.o, self.desc, c), c.q0, self.opts, max_iter)
        return self._refs[i, max_iter]


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    c = Ctx(_capi, oracle_mod)
    yield c
    c.h.close()


def _bits(res):
    return tuple(np.asarray(x).tobytes() for x in res)


# ------------------------------------------------------------------------------------------ 1. value at the seed
def test_value_at_seed(ctx):
    worst = 0.0
    for i, (c, (q, cost, it, st)) in enumerate(zip(ctx.cases, ctx.run(0))):
        assert (it, st) == (0, ref.GTO_STATUS_MAX_ITER), c
        assert q.tobytes() == ctx.qc[i].tobytes(), c   # the seed, clipped (q_clip: sx and the flap) and otherwise unchanged
        want = ref.pose_term(c.kind, ctx.T[i], c.goal)
        tol = 1e-10 * abs(want) + 1e-14 + c.allow_value
        worst = max(worst, abs(cost - want) / tol)
        print(f"{c.name:24s} cost {cost:.17g} restatement {want:.17g} difference {cost - want:+.3e} bound {tol:.3e}")
        assert abs(cost - want) <= tol, c
    print(f"largest share of the bound used: {worst:.3f}")


# ------------------------------------------------------------------------------------------ 2. first step
def test_first_step(ctx):
    for i, (c, (q, cost, it, st)) in enumerate(zip(ctx.cases, ctx.run(1))):
        if c.on_clamp:
            continue
        qr, fr, itr, str_ = ctx.ref(i, 1)
        err = np.abs(q - qr).max()
        print(f"{c.name:24s} iters {it} status {st} (restatement {itr} {str_}) |q - q_ref| {err:.3e} bound {1e-9 + c.allow_step:.3e}")
        assert (it, st) == (itr, str_), c
        assert err <= 1e-9 + c.allow_step, c


# ------------------------------------------------------------------------------------------ 3. lock-step to the end
def test_lockstep_to_the_end(ctx):
    n = 0
    for i, (c, (q, cost, it, st)) in enumerate(zip(ctx.cases, ctx.run(50))):
        if not c.lockstep:
            continue
        qr, fr, itr, str_ = ctx.ref(i, 50)
        print(f"{c.name:24s} iters {it} status {st} (restatement {itr} {str_}) |q - q_ref| {np.abs(q - qr).max():.3e} cost {cost:.6e} {fr:.6e}")
        assert (it, st) == (itr, str_), c
        np.testing.assert_allclose(q, qr, rtol=0, atol=1e-9, err_msg=c.name)
        np.testing.assert_allclose(cost, fr, rtol=1e-10, atol=1e-15, err_msg=c.name)
        n += 1
    assert n >= 53


# ------------------------------------------------------------------------------------------ 4. the other cases, solved
def test_full_solve_of_the_cases_without_a_lockstep(ctx):
    """On the clamp, within 1e-3 of it and within 1e-6 of a cut the restatement's own path depends on the last bits of the
    frame (see the allowances): the solve must stay finite, end in a regular status and not end above where it began."""
    n = 0
    for c, (q, cost, it, st), (_, cost0, _, _) in zip(ctx.cases, ctx.run(50), ctx.run(0)):
        if c.lockstep:
            continue
        assert np.isfinite(q).all() and np.isfinite(cost), c
        assert st in OK, c
        assert cost <= cost0, c
        n += 1
    assert n >= 14


# ------------------------------------------------------------------------------------------ 5. sign and scale of the goal
def test_goal_quaternion_sign_and_scale(ctx):
    by = {c.name: i for i, c in enumerate(ctx.cases)}
    twins = 0
    for max_iter in (0, 1, 50):
        res = ctx.run(max_iter)
        for i, c in enumerate(ctx.cases):
            if c.twin:
                assert _bits(res[i]) == _bits(res[by[c.twin]]), (c, max_iter)
                twins += 1
    assert twins >= 3 * 16
    i = by["q_zero"]
    c = ctx.cases[i]
    pos = float(np.sum((ctx.T[i][:3, 3] - c.goal[:3]) ** 2))
    np.testing.assert_allclose(ctx.run(0)[i][1], pos + 1.0, rtol=1e-10, atol=1e-14)
    # its first step is the position term's alone: the restatement's, whose orientation rows are all zero at this goal
    # (tests/test_ik_pose_cases_cpu.py); the value after it is the new position term plus the same 1
    q1, f1, it, st = ctx.run(1)[i]
    qr, fr, itr, str_ = ctx.ref(i, 1)
    assert (it, st) == (itr, str_) and np.abs(q1 - qr).max() <= 1e-9
    T1 = ctx.o.eval_fk(q1[None])[0, ctx.fe]
    np.testing.assert_allclose(f1, float(np.sum((T1[:3, 3] - c.goal[:3]) ** 2)) + 1.0, rtol=1e-10, atol=1e-14)
    assert f1 < pos + 1.0 and np.abs(q1 - ctx.qc[i]).max() > 1e-2
    # scaled goals: the restatement's value, |p - g|^2 + 1 - (q . g)^2 with the norm in it
    for name in ("q_scaled_half", "q_scaled_double"):
        j = by[name]
        np.testing.assert_allclose(ctx.run(0)[j][1], ref.reference_pose_term(Q, ctx.T[j], ctx.cases[j].goal), rtol=1e-10, atol=1e-14)


# ------------------------------------------------------------------------------------------ 6. ancestor mask
def test_joint_beside_the_chain_without_a_scene(ctx):
    """No residual depends on the flap: it keeps its clipped seed value bit for bit (q_clip starts beyond its limit), and the
    solve goes on as the restatement's does: iterations and status are the restatement's wherever a step is compared at all
    (one step: every case off the clamp; 50: the lock-step cases).  The other cases (on the clamp, within 1e-3 of it, within
    1e-6 of a cut) are the ones whose path the restatement itself does not keep under +-ETA: a regular status is asked."""
    for max_iter in (0, 1, 50):
        for i, (c, (q, cost, it, st)) in enumerate(zip(ctx.cases, ctx.run(max_iter))):
            assert q[ipc.J_FLAP].tobytes() == ctx.qc[i, ipc.J_FLAP].tobytes(), (c, max_iter)
            assert q[ipc.J_TAB].tobytes() == ctx.q0[i, ipc.J_TAB].tobytes(), (c, max_iter)
            if max_iter and (c.lockstep or (max_iter == 1 and not c.on_clamp)):
                assert (it, st) == ctx.ref(i, max_iter)[2:], (c, max_iter)
            assert st in OK, (c, max_iter)


def test_joint_beside_the_chain_with_a_scene(ctx):
    """With a cost field the flap's link is pushed: the joint has a gradient and no curvature, and moves."""
    res = ctx.run(50, scene=True)
    q = np.stack([r[0] for r in res])
    cost = np.array([r[1] for r in res])
    assert np.isfinite(q).all() and np.isfinite(cost).all()
    assert all(r[3] in OK for r in res)
    T = ctx.o.eval_fk(q)[:, ctx.fe]
    _, _, val, _ = ctx.o.eval_points(0, q, [0.0, 0.0, 0.0], use_obs=True)
    want = np.array([ref.pose_term(c.kind, T[i], c.goal) for i, c in enumerate(ctx.cases)]) + ctx.opts.w_obstacle * val.sum(axis=1)
    for i, c in enumerate(ctx.cases):
        print(f"{c.name:24s} cost {cost[i]:.17g} pose + collision at the returned q {want[i]:.17g}")
    np.testing.assert_allclose(cost, want, rtol=1e-9, atol=1e-13)
    moved = np.abs(q[:, ipc.J_FLAP] - ctx.qc[:, ipc.J_FLAP])
    print(f"the flap moved in {int((moved > 1e-6).sum())} of {len(res)} cases, by up to {moved.max():.3f} rad")
    assert (moved > 1e-3).any()
    assert np.array_equal(q[:, ipc.J_TAB], ctx.q0[:, ipc.J_TAB])
    _, cost0, _, _ = zip(*ctx.run(0, scene=True))
    assert np.all(cost <= np.array(cost0))


def test_point_goal_with_a_joint_beside_the_chain_matches_oracle(ctx):
    """gto_solve_ik_batch (kind 0) shares the step with the pose kinds: on this robot against the oracle's solve_ik_batch,
    held as tests/test_gpu_parity.py::test_ik_matches_oracle holds the built-in arms."""
    ids = [i for i, c in enumerate(ctx.cases) if c.goal_pose is not None and c.twin is None][:12]
    goals = np.stack([ctx.cases[i].goal_pose for i in ids]).reshape(-1, 16)
    q0 = ctx.q0[ids]
    for sid in (None, 0):
        qg, fg, itg, stg = ctx.h.solve_ik_batch(sid, q0, goals, np.zeros((len(ids), 3)), max_iter=50)
        qo, fo, ito, sto = ctx.o.solve_ik_batch(sid, q0, goals, np.zeros((len(ids), 3)), max_iter=50)
        np.testing.assert_array_equal(itg, ito)
        np.testing.assert_array_equal(stg, sto)
        assert np.isin(stg, OK).all()
        np.testing.assert_allclose(qg, qo, rtol=0, atol=1e-6)
        np.testing.assert_allclose(fg, fo, rtol=1e-8, atol=1e-12)
        if sid is None:
            assert np.array_equal(qg[:, ipc.J_FLAP], ctx.qc[ids, ipc.J_FLAP])


# ------------------------------------------------------------------------------------------ 7. batch position
def test_batch_position(ctx):
    n = len(ctx.cases)
    fwd = ctx.run(50)
    rev = ctx.solve(list(range(n))[::-1], 50)[::-1]
    for i, c in enumerate(ctx.cases):
        assert _bits(fwd[i]) == _bits(rev[i]), c
        assert _bits(fwd[i]) == _bits(ctx.solve([i], 50)[0]), c
