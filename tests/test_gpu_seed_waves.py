"""GPU: gto_seed_goalsets_device and gto_ik_report_device where tests/test_gpu_grasp_chain.py does not reach: goal sets wider
than one wave (k_seed_score and k_seed_select walk a set 64 rows at a time: tests/seed_cases.py puts the accepted rows, the
ties, the NaNs and the cheapest row across the chunks), the obstacle cost of every candidate against the FP64 CPU oracle
(Oracle.plan_cost) rather than against gto_plan_cost alone, horizons whose last group of GTO_PLAN_TG = 4 waypoints holds 1, 2
or 3, the largest horizon, and random and 32-frame trees with prismatic optimised joints and many parameter joints.  Run the
file under a time limit (timeout -k 10 900 pytest ...) and stop at the first fault."""
import numpy as np
import pytest

import grasp_chain_ref as ref
from grasptrajopt_amd import synthetic as syn
from helpers import Problem, limit_robot, random_robot
from seed_cases import WIDE_B, seed_case_wide, wide_rows
from test_gpu_grasp_chain import (IK_ITERS, chain_setup, chain_thresholds, cu, dev_empty, host_chain, run_seeds, same_bits,
                                  widest_gap)

pytestmark = pytest.mark.gpu

RT_COST, RT_DIST = 1e-12, 1e-14  # what test_plan_cost_vs_oracle holds k_plan_cost to


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as gr
    gr.build()
    from grasptrajopt_amd import _capi
    return _capi


class Rig:
    """A HIP handle and the oracle of one robot at one horizon, two scenes set on both."""

    def __init__(self, capi, oracle_mod, desc, ee, gripper, T, offset, qc0, **kw):
        self.desc, self.T, self.offset, self.qc0 = desc, T, offset, np.asarray(qc0, dtype=np.float64)
        opts = oracle_mod.reference_opts(T=T, standoff_offset=offset)
        self.h = capi.SolverHandle(desc, ee, gripper, opts, device=0, **kw)
        self.o = oracle_mod.Oracle(desc, ee, gripper, opts, **kw)
        self.fe = desc.frame_index(ee)

    def set_scenes(self, scenes):
        for sid, sc in enumerate(scenes):
            for s in (self.h, self.o):
                s.set_scene(sid, sc.c_all, sc.c_obs, sc.shape, sc.origin, sc.res)


def panda_rig(capi, oracle_mod, T=50, offset=-10):
    """A table scene and a shelf scene, the table top and the lower board at -0.06 m: the base link, which no candidate
    moves, stays above the cost band whatever the base offset (+-0.03 m) and in front of the shelf.  A link that stands in
    the band adds the same cost to every candidate, the cheapest ones would tie in cost exactly, and whether their order
    survives a rounding of the sum could not be told from the tolerance."""
    scenes = [Problem("panda", B=1, scene_seed=5, T=T, table_z=-0.06), Problem("panda", B=1, scene_seed=9, T=T, table_z=-0.06, shelf=True)]
    prob = scenes[0]
    rig = Rig(capi, oracle_mod, prob.desc, prob.cfg["link_ee"], prob.cfg["link_gripper"], T, offset, prob.qc[0])
    rig.set_scenes([p.scene for p in scenes])
    return rig


def scenes_around(rig, q, base, per=1):
    """Two synthetic scenes (syn.make_scene) for a robot that is not one of the built-in arms: the table top 2 cm (the width
    of the cost band) below the median, over groups of `per` consecutive configurations of q, of the group's lowest surface
    point, so that about half of the groups stay clear of it; and low enough that a surface point that is the same in every
    configuration (a link no optimised joint moves) stays above the band at any base offset within +-0.03 m, for the reason
    given in panda_rig.  The grid spans 2.2 m around the base."""
    z = rig.o.eval_points(0, q, base, want_field=False)[0][:, :, 2]
    table_z = float(np.median(z.min(axis=1).reshape(-1, per).min(axis=1))) - 0.02
    still = z.max(axis=0) - z.min(axis=0) < 1e-9
    if still.any():
        table_z = min(table_z, float(z[0, still].min()) - 0.06 - 0.02 - 1e-3)
    return [syn.make_scene(seed, n=48, res=0.0467, origin=(-1.12, -1.12, table_z - 1.0), table_z=table_z) for seed in (5, 9)]


def other_robot(name):
    if name == "bushy":
        return limit_robot("bushy", n_opt=8) + (50, -10)
    return random_robot(int(name)) + (22, -4)  # 22 waypoints: a last group of 2


def other_rig(capi, oracle_mod, name):
    desc, ee, T, offset = other_robot(name)
    rng = np.random.default_rng(17)
    return Rig(capi, oracle_mod, desc, ee, ee, T, offset, rng.uniform(0.3 * desc.lower, 0.3 * desc.upper), n_gripper_points=40)


OTHER_ROBOTS = ["3", "7", "9", "bushy"]  # random_robot(3): 21 frames, 13 parameter joints; (7): 24 frames; (9): 8 optimised joints


def test_the_other_robots_are_what_they_are_chosen_for():
    descs = [other_robot(name)[0] for name in OTHER_ROBOTS]
    assert all(d.n_opt <= 8 for d in descs)

    def prismatic_optimised(d):
        return any(d.joint_type[f] == 2 and d.q_index[f] in set(d.opt_index.tolist()) for f in range(d.n_frames))
    assert any(prismatic_optimised(d) for d in descs[:3]) and any(d.n_frames >= 20 for d in descs[:3])
    assert descs[3].n_frames == 32 and prismatic_optimised(descs[3]) and len(descs[0].param_index) >= 10


# ------------------------------------------------------------------------------------------------- seeds
def oracle_lowest(rig, sid, base, f32=False):
    """seed_cases' `lowest`: the row np.lexsort((dist, cost)) of the oracle's scores puts first."""
    def lowest(b, qc, qs):
        plans = ref.candidates(qc, qs, rig.T, rig.desc.param_index, f32)
        return ref.choose(rig.o.plan_cost(int(sid[b]), plans, base[b])[0], ref.distance(plans))
    return lowest


def wide_case(rig, n_max, seed, instances=None, lowest=True):
    """seed_case_wide with the oracle as the scorer.  Scene ids and bases do not depend on `lowest`: a first draw with the
    stand-in scorer yields them (the same generator state draws the same ones again)."""
    first = seed_case_wide(rig.desc, rig.qc0, np.random.default_rng(seed), n_max, instances=instances)
    if not lowest:
        return first
    sid, base = seed_case_wide(rig.desc, rig.qc0, np.random.default_rng(seed), n_max)[5:]
    case = seed_case_wide(rig.desc, rig.qc0, np.random.default_rng(seed), n_max, oracle_lowest(rig, sid, base), instances)
    assert case[5].tobytes() == first[5].tobytes() and case[6].tobytes() == first[6].tobytes()
    return case


def oracle_seeds(rig, case, f32):
    """Per instance the restatement with the oracle's plan_cost as the score (Q0 left aside: it is rebuilt per call)."""
    qc, qs, goals, n_goals, accept, sid, base = case
    out = []
    for b in range(len(qc)):
        got = {}

        def score(plans, b=b, got=got):
            got["cost"], got["dist"] = rig.o.plan_cost(int(sid[b]), plans, base[b])
            return got["cost"]
        r = ref.seed_goalsets(qc[b], goals[b], n_goals[b], qs[b], accept[b], rig.T, rig.offset, rig.desc.param_index, True, f32, score)
        r["oracle_dist"] = got.get("dist", np.empty(0))
        out.append(r)
    return out


def keys_equal(c1, d1, c2, d2):
    return (c1 == c2 or (c1 != c1 and c2 != c2)) and (d1 == d2 or (d1 != d1 and d2 != d2))


def clearly_first(cost, dist):
    """Whether every scorer within RT_COST, RT_DIST of (cost, dist) makes the choice np.lexsort((dist, cost))[0] makes.  The
    candidates that share the first key bit for bit are copies of one solution (a kernel scores them bit-equal too, which
    the test asserts on its own): the lowest position wins among them whatever the rounding.  Of the others only the next
    key in the order matters.  It is clear of the first if its cost is above by more than the two tolerances together; or if
    both costs are exactly 0 (a relative tolerance keeps a zero a zero) and its distance is above in the same way; a NaN is
    behind every number in both scorers (the NaNs sit in the same places)."""
    order = np.lexsort((dist, cost))
    c0, d0 = cost[order[0]], dist[order[0]]
    rest = [k for k in order[1:] if not keys_equal(cost[k], dist[k], c0, d0)]
    if not rest:
        return True
    c1, d1 = cost[rest[0]], dist[rest[0]]

    def above(a1, a0, rt):
        return a0 == a0 and (a1 != a1 or a1 - a0 > 2.0 * rt * (abs(a1) + abs(a0)))
    return bool(above(c1, c0, RT_COST) or (c1 == 0.0 and c0 == 0.0 and above(d1, d0, RT_DIST)))


def check_seeds(rig, case, want, interpolate, f32, ties_at=()):
    """One call of gto_seed_goalsets_device against the oracle-scored restatement `want`.  Returns the number of instances
    left out of the comparison of the choice with the oracle's, and the largest relative difference of seed_cost from the
    oracle."""
    import torch
    h, d, T = rig.h, rig.desc, rig.T
    qc, qs, goals, n_goals, accept, sid, base = case
    B, n_max = qs.shape[:2]
    got = run_seeds(h, torch, T, qc, qs, goals, n_goals, accept, sid, base, interpolate, f32)
    left_out, worst = 0, 0.0
    for b in range(B):
        r = want[b]
        na = r["n_accepted"]
        assert got["n_accepted"][b] == na and got["n_goals_out"][b] == r["n_goals_out"], b
        assert got["goals_out"][b, :r["n_goals_out"]].tobytes() == r["goals_out"].tobytes(), b
        assert (got["goals_out"][b, r["n_goals_out"]:] == -7.0).all(), b                                             # untouched
        assert (got["seed_cost"][b, na:] == -7.0).all() and (got["seed_dist"][b, na:] == -7.0).all(), b
        if na == 0:
            assert got["seed_index"][b] == -1 and got["Q0"][b].tobytes() == np.tile(qc[b][:, None], (1, T)).tobytes(), b
            continue
        g_cost, g_dist = got["seed_cost"][b, :na], got["seed_dist"][b, :na]
        o_cost, o_dist = r["seed_cost"], r["oracle_dist"]
        # the FP64 oracle
        assert np.array_equal(np.isnan(g_cost), np.isnan(o_cost)) and np.array_equal(np.isnan(g_dist), np.isnan(o_dist)), b
        fin = np.isfinite(o_cost) & (o_cost != 0.0)
        if fin.any():
            worst = max(worst, float((np.abs(g_cost[fin] - o_cost[fin]) / np.abs(o_cost[fin])).max()))
        np.testing.assert_allclose(g_cost, o_cost, rtol=RT_COST, atol=0, err_msg=str(b))
        np.testing.assert_allclose(g_dist, o_dist, rtol=RT_DIST, atol=0, err_msg=str(b))
        # gto_plan_cost of the host-built candidates, bit for bit (a NaN distance is a NaN on both sides)
        h_cost, h_dist = h.plan_cost(int(sid[b]), r["plans"], base[b])
        assert g_cost.tobytes() == h_cost.tobytes(), b
        assert same_bits(g_dist, h_dist) and same_bits(r["seed_dist"], h_dist), b
        # the choice: exact on the kernel's own scores, the oracle's where rounding cannot turn it
        k = int(got["seed_index"][b])
        assert k == int(np.lexsort((g_dist, g_cost))[0]), (b, k)
        if clearly_first(o_cost, o_dist):
            assert k == r["seed_index"], (b, k, r["seed_index"])
        else:
            left_out += 1
        if b in ties_at:  # every row accepted: position = row
            assert na == n_max
            for rows in (wide_rows(n_max)["ties3"], wide_rows(n_max)["ties2"]):
                for x in (g_cost, g_dist):
                    assert all(x[p].tobytes() == x[rows[0]].tobytes() for p in rows), (b, rows)
        Q0 = ref.seed_from(qc[b], r["plans"][k], interpolate, T, rig.offset)
        assert got["Q0"][b].tobytes() == Q0.tobytes(), b
    # accept = NULL: every row counts
    allg = run_seeds(h, torch, T, qc, qs, goals, n_goals, None, sid, base, interpolate, f32)
    ones = run_seeds(h, torch, T, qc, qs, goals, n_goals, np.ones_like(accept), sid, base, interpolate, f32)
    for key in allg:
        assert allg[key].tobytes() == ones[key].tobytes(), key
    assert (allg["n_accepted"] == np.clip(n_goals, 1, n_max)).all()
    # any position in any batch: reversed, and one instance on its own
    rev = run_seeds(h, torch, T, *[x[::-1].copy() for x in case], interpolate, f32)
    for key in got:
        assert rev[key][::-1].tobytes() == got[key].tobytes(), key
    alone = min(8, B - 1)
    one = run_seeds(h, torch, T, *[x[alone:alone + 1].copy() for x in case], interpolate, f32)
    for key in got:
        assert one[key].tobytes() == got[key][alone:alone + 1].tobytes(), key
    return left_out, worst


@pytest.fixture(scope="module")
def panda50(capi, oracle_mod):
    rig = panda_rig(capi, oracle_mod)
    rig.cases = {}
    yield rig
    rig.h.close()


@pytest.mark.parametrize("n_max", [63, 64, 65, 128, 130, 200])
@pytest.mark.parametrize("interpolate", [True, False])
@pytest.mark.parametrize("f32", [True, False])
def test_seeds_wider_than_a_wave(panda50, n_max, interpolate, f32):
    """The twelve instances of seed_cases.seed_case_wide on Panda at T = 50.  By the oracle alone no instance is left out of
    the comparison of the choice at n_max = 63 .. 130 and one of twelve at 200; the test prints the count and the largest
    relative difference of seed_cost from the oracle."""
    rig = panda50
    if n_max not in rig.cases:  # the case and the oracle's scores of it, once for the four calls
        case = wide_case(rig, n_max, seed=100 + n_max)
        rig.cases[n_max] = (case, {f: oracle_seeds(rig, case, f) for f in (True, False)})
    case, want = rig.cases[n_max]
    qs, accept, n_goals = case[1], case[4], case[3]
    # the generator's promises about scores, by the oracle: 7's tied solution and 8's far row are the cheapest
    R = wide_rows(n_max)
    assert want[False][7]["seed_index"] == 3
    assert ref.accepted_rows(n_goals[8], n_max, accept[8])[want[False][8]["seed_index"]] == R["far"]
    assert np.isnan(want[f32][9]["oracle_dist"][list(R["nans"])]).all() and want[f32][9]["seed_index"] not in R["nans"]
    cost = np.concatenate([w["seed_cost"] for w in want[f32]])
    assert (cost > 0).any() and (cost == 0).any()
    left_out, worst = check_seeds(rig, case, want[f32], interpolate, f32, ties_at=(6, 7))
    print(f"seeds n_max={n_max} interpolate={interpolate} f32={f32}: {left_out} of {WIDE_B} instances left out of the oracle's choice, "
          f"max rel seed_cost diff from the oracle {worst:.3e}")
    assert left_out <= 1


REDUCED = (0, 1, 2, 6, 9, 10)


def reduced_check(rig):
    n_max = 70
    case = wide_case(rig, n_max, seed=170, instances=REDUCED, lowest=False)
    for f32 in (True, False):
        want = oracle_seeds(rig, case, f32)
        cost = np.concatenate([w["seed_cost"] for w in want])
        assert (cost > 0).any() and (cost == 0).any()
        for interpolate in (True, False):
            left_out, worst = check_seeds(rig, case, want, interpolate, f32, ties_at=(REDUCED.index(6),))
            print(f"seeds {rig.desc.name} T={rig.T} ts={rig.T + rig.offset} interpolate={interpolate} f32={f32}: {left_out} of "
                  f"{len(REDUCED)} left out, max rel seed_cost diff from the oracle {worst:.3e}")
            assert left_out <= 1


HORIZONS = {"T5": (5, -1), "T7": (7, -5), "T96": (96, -40)}  # ts = T - 1; ts = 2; the largest horizon


@pytest.mark.parametrize("which", list(HORIZONS) + OTHER_ROBOTS)
def test_seeds_other_horizons_and_robots(capi, oracle_mod, which):
    """Panda with a last group of 1 waypoint (T = 5), of 3 (T = 7) and at the largest horizon; random trees (T = 22: a last
    group of 2) and the bushy 32-frame tree (T = 50): branching, prismatic optimised joints, up to 16 parameter joints whose
    solution values must not count.  A candidate of these robots is scored in a scene laid around its own reach."""
    if which in HORIZONS:
        T, offset = HORIZONS[which]
        assert 2 <= T + offset <= T - 1
        rig = panda_rig(capi, oracle_mod, T, offset)
    else:
        rig = other_rig(capi, oracle_mod, which)
        case = wide_case(rig, 70, seed=170, instances=REDUCED, lowest=False)
        plans = ref.candidates(case[0][0], case[1][0], rig.T, rig.desc.param_index)  # instance 0: every row
        q = np.ascontiguousarray(plans.transpose(0, 2, 1)).reshape(-1, rig.desc.ndof)
        rig.set_scenes(scenes_around(rig, q, case[6][0], per=rig.T))
    reduced_check(rig)
    rig.h.close()


# ------------------------------------------------------------------------------------------------- report
@pytest.mark.parametrize("name", OTHER_ROBOTS)
def test_report_on_other_robots_against_the_oracle(capi, oracle_mod, name):
    """err_pos to 1e-12 m, err_rot to 1e-5 degrees, cost to relative 1e-11 against grasp_chain_ref.report of the oracle's
    eval_fk and eval_points, at 130 instances; accept equal on every instance with thresholds the oracle's values stay clear
    of.  The first four goals are the oracle's own frames: the trace of R_goal^T R is 3 up to rounding, on either side of it."""
    import torch
    B = 130
    rig = other_rig(capi, oracle_mod, name)
    d, h, o = rig.desc, rig.h, rig.o
    rng = np.random.default_rng(31)
    q = rng.uniform(d.lower, d.upper, (B, d.ndof))
    base = rng.uniform(-0.03, 0.03, (B, 3))
    sid = (np.arange(B) % 2).astype(np.int32)
    rig.set_scenes(scenes_around(rig, q, base))
    off = rng.uniform(-1.0, 1.0, (B, d.ndof)) * np.linspace(0.0, 0.3, B)[:, None] * (d.upper - d.lower)[None, :]
    off[:4] = 0.0
    tf_o = o.eval_fk(q)[:, rig.fe]
    RT = o.eval_fk(np.clip(q + off, d.lower, d.upper))[:, rig.fe]
    assert RT[:4].tobytes() == tf_o[:4].tobytes()
    cost_o = np.stack([o.eval_points(int(sid[b]), q[b:b + 1], base[b], use_obs=True)[2].sum(axis=1)[0] for b in range(B)])
    assert (cost_o > 0).any() and (cost_o == 0).any()
    ep_o, er_o, _ = ref.report(tf_o, RT, cost_o, 1.0, 1.0, 1.0)
    assert (ep_o[:4] == 0).all() and (er_o[:4] < 1e-5).all()
    pos_tol, m_pos = widest_gap(ep_o, 1e-3)
    rot_tol, m_rot = widest_gap(er_o, 1e-2)
    cost_tol, m_cost = widest_gap(cost_o, 1.0)
    assert m_pos > 1e-9 and m_rot > 1e-3 and m_cost > 1e-9 * max(1.0, np.abs(cost_o).max())
    acc = ref.report(tf_o, RT, cost_o, pos_tol, rot_tol, cost_tol)[2]
    assert 0 < acc.sum() < B
    outs = [dev_empty((B,), torch.float64) for _ in range(3)] + [dev_empty((B,), torch.uint8, 9)]
    keep = [cu(sid), cu(q), cu(RT.reshape(B, 16)), cu(base)]
    torch.cuda.synchronize()
    h.ik_report_device(B, *[x.data_ptr() for x in keep], pos_tol, rot_tol, cost_tol, *[x.data_ptr() for x in outs])
    torch.cuda.synchronize()
    g_ep, g_er, g_cost, g_acc = [x.cpu().numpy() for x in outs]
    print("report", d.name, "max |err_pos diff|", np.abs(g_ep - ep_o).max(), "max |err_rot diff|", np.abs(g_er - er_o).max(),
          "max rel cost diff", (np.abs(g_cost - cost_o) / np.maximum(np.abs(cost_o), 1e-300)).max(), "err_rot[:4]", g_er[:4])
    assert not np.isnan(g_er).any()
    np.testing.assert_allclose(g_ep, ep_o, rtol=0, atol=1e-12)
    np.testing.assert_allclose(g_er, er_o, rtol=0, atol=1e-5)
    np.testing.assert_allclose(g_cost, cost_o, rtol=1e-11, atol=0)
    assert np.array_equal(g_acc.astype(bool), acc)
    h.close()


# ------------------------------------------------------------------------------------------------- the chain
def test_chain_with_seventy_grasps_is_the_host_composed_chain():
    """test_chain_on_one_object_is_the_host_composed_chain with a goal set of 70: accepted grasps in both chunks."""
    from grasptrajopt_amd.grasp_chain import GraspChain
    n, interpolate, max_iter = 70, True, 10
    cfg, robot, fields, RT = chain_setup("panda", n, seed=21)
    qc = np.array(cfg["default_pose"], dtype=np.float64)
    base = np.array([0.01, -0.02, 0.0])
    ik_RT = RT @ syn.standoff_pose(-0.1, cfg["axis_standoff"])
    pos_tol, rot_tol, cost_tol = chain_thresholds(robot, cfg, qc, ik_RT, fields[0], base)
    want = host_chain(robot, cfg, qc, ik_RT, RT, fields[0], base, interpolate, pos_tol, rot_tol, cost_tol, max_iter)
    assert 0 < want["accept"].sum() < n and want["accept"][:64].any() and want["accept"][64:].any()
    assert not want["accept"][:64].all()
    chain = GraspChain(robot, cfg["link_ee"], cfg["link_gripper"], standoff_distance=-0.1, standoff_offset=-10)
    chain.max_iter, chain.ik_max_iter = max_iter, IK_ITERS
    r = chain.plan_objects(qc, ik_RT[None], RT[None], [n], fields[0], base, axis_standoff=cfg["axis_standoff"], interpolate=interpolate,
                           pos_tol=pos_tol, rot_tol_deg=rot_tol, ik_collision_threshold=cost_tol)
    assert r.q_solutions.dtype == np.float32 and r.q_solutions[0].tobytes() == want["q"].astype(np.float32).tobytes()
    np.testing.assert_allclose(r.err_pos[0], want["err_pos"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(r.err_rot[0], want["err_rot"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(r.ik_cost[0], want["ik_cost"], rtol=1e-11, atol=0)
    assert np.array_equal(r.accept[0], want["accept"]) and r.n_accepted[0] == want["accept"].sum()
    assert r.seed_index[0] == want["seed_index"]
    assert r.plans[0].tobytes() == want["plan"].tobytes() and r.dQ[0].tobytes() == want["dQ"].tobytes()
    assert r.cost.tobytes() == want["f"].tobytes() and r.iters[0] == want["iters"]
    chain.close()
    robot.close()
