"""GPU: gto_self_clearance against its numpy restatement (tests/self_clearance_ref.py), bit for bit.

The reference runs on the world points h.eval_points returns at base 0, so the comparison is of the statistic alone: d2 and
pair must be EQUAL.  Sections:
  1. Panda, Fetch and one column of panda_5k under every mask of the shared table; B = 1, 3, 65 and Tp = 1, GTO_CHECK_TG + 1,
     50 are batches of the same columns, every GTO_CHECK_TG included
  2. cutoffs: each result equals min(the result without a cutoff, c*c) with pair -1 where far: what pins the culling
  3. the smallest robots: a one-point link, a link of 65 points (two chunks that must never meet), static links only, chain_1
  4. a NaN and an Inf column inside a path at batch positions 0, 1 and 64
  5. the host entry point equals the device entry point; the device call behind a busy stream
  6. the chain and the planner report what the calls one by one return
"""
import numpy as np
import pytest

import held_stream as hs
import self_clearance_ref as R
import small_robots as sr

pytestmark = pytest.mark.gpu
CHECK_TG = 4  # GTO_CHECK_TG (csrc/gto_observe.h)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class Rig:
    """A robot's handle, its columns, their world points (h.eval_points at base 0) and the reference per mask, computed
    once and shared."""

    def __init__(self, capi, robot):
        from grasptrajopt_amd.robot_desc import load_builtin
        self.robot, self.desc = robot, load_builtin(robot)
        cfg = R.config(robot)
        self.h = capi.SolverHandle(self.desc, cfg["link_ee"], cfg["link_gripper"], device=0)
        self.q = R.robot_columns(robot, self.desc)
        self.X = self.h.eval_points(0, self.q, [0.0, 0.0, 0.0], want=("xyz",))[0]
        self.masks = R.masks(robot, self.desc)
        self.clearance = self.desc.point_spacing()
        self._want = {}

    def want(self, mask_name):
        """(d2 (n,), pair (n, 2)) of the columns under a mask, without a cutoff."""
        if mask_name not in self._want:
            d2, pair = R.reference_paths(self.X[None], self.desc.point_link, self.masks[mask_name])
            self._want[mask_name] = (d2[0], pair[0])
        return self._want[mask_name]

    def paths(self, B, Tp):
        """(paths (B, ndof, Tp), column index (B, Tp)): the robot's columns dealt out in an order that differs per shape."""
        n = len(self.q)
        idx = (np.arange(B * Tp) * 7 + B + Tp) % n
        idx = idx.reshape(B, Tp)
        return np.ascontiguousarray(self.q[idx].transpose(0, 2, 1)), idx


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def rigs(capi):
    made = {}

    def get(robot):
        if robot not in made:
            made[robot] = Rig(capi, robot)
        return made[robot]
    yield get
    for r in made.values():
        r.h.close()


# ---------------------------------------------------------------------------------------------- 1. robots, masks, shapes
@pytest.mark.parametrize("robot", R.ROBOTS)
def test_every_mask_equals_the_restatement(rigs, robot):
    r = rigs(robot)
    paths = np.ascontiguousarray(r.q.T[None])  # one path whose columns are the robot's columns
    for name, M in r.masks.items():
        r.h.set_self_pairs(M)
        got = r.h.self_clearance(paths)
        d2, pair = r.want(name)
        print(robot, name, "dist", np.round(np.sort(np.sqrt(d2))[:4], 4), "pairs", sorted({tuple(p) for p in pair.tolist()}))
        assert same(got["d2"][0], d2) and same(got["pair"][0], pair), name
        assert same(got["dist"], np.sqrt(got["d2"]))
    d2, pair = r.want("empty")
    assert np.isinf(d2).all() and (pair == -1).all()
    r.h.set_self_pairs(None)


def test_panda_5k_column(rigs):
    r = rigs("panda_5k")
    for name in ("default", "unset"):
        r.h.set_self_pairs(r.masks[name])
        got = r.h.self_clearance(np.ascontiguousarray(r.q.T[None]))
        d2, pair = r.want(name)
        assert same(got["d2"][0], d2) and same(got["pair"][0], pair), name
    r.h.set_self_pairs(None)


@pytest.mark.parametrize("robot", R.ROBOTS)
def test_batches_and_lengths_and_columns_per_workgroup(rigs, monkeypatch, robot):
    r = rigs(robot)
    r.h.set_self_pairs(r.masks["default"])
    d2, pair = r.want("default")
    for B in (1, 3, 65):
        for Tp in (1, CHECK_TG + 1, 50):
            paths, idx = r.paths(B, Tp)
            got = r.h.self_clearance(paths)
            assert same(got["d2"], d2[idx]) and same(got["pair"], pair[idx]), (B, Tp)
    paths, idx = r.paths(3, CHECK_TG + 3)
    for tg in ("1", "2", "3", "4"):
        monkeypatch.setenv("GTO_CHECK_TG", tg)
        got = r.h.self_clearance(paths, cutoff=2 * r.clearance)
        wd2, wpair = R.apply_cutoff(d2[idx], pair[idx], 2 * r.clearance)
        assert same(got["d2"], wd2) and same(got["pair"], wpair), tg
    monkeypatch.delenv("GTO_CHECK_TG")
    r.h.set_self_pairs(None)


# ---------------------------------------------------------------------------------------------- 2. cutoffs
@pytest.mark.parametrize("robot", R.ROBOTS + ("panda_5k",))
@pytest.mark.parametrize("mask", ["default", "far", "unset"])
def test_a_cutoff_is_the_minimum_with_its_square(rigs, robot, mask):
    r = rigs(robot)
    r.h.set_self_pairs(r.masks[mask])
    paths = np.ascontiguousarray(r.q.T[None])
    d2, pair = r.want(mask)
    # (panda_5k has one column: "between" is then twice its distance, "below" half of it)
    for c in R.cutoffs(np.sqrt(d2), r.clearance):
        got = r.h.self_clearance(paths, cutoff=c)
        wd2, wpair = R.apply_cutoff(d2, pair, c)
        print(robot, mask, f"cutoff {c:.4f}: {int((wpair[:, 0] >= 0).sum())} of {len(d2)} columns near")
        assert same(got["d2"][0], wd2) and same(got["pair"][0], wpair), c
    r.h.set_self_pairs(None)


# ---------------------------------------------------------------------------------------------- 3. the smallest robots
def small_robot(kind):
    """(desc, link_ee, link_gripper) of a robot small enough to go wrong."""
    if kind == "link_of_65":  # three links on a 2-joint chain; the first has 65 points: two chunks of one link
        return sr._tree(kind, 5, [-1, 0, 1], [0, 1, 1], [0, 1, 2], [65, 1, 7]), "f2", "f2"
    if kind == "one_point_links":  # every link one point
        return sr._tree(kind, 6, [-1, 0, 1], [0, 1, 1], [0, 1, 2], [1, 1, 1]), "f2", "f2"
    rb = sr.Robot(kind)
    return rb.desc, rb.ee, rb.gripper


@pytest.mark.parametrize("kind", ["link_of_65", "one_point_links", "one_point", "static_links_only", "chain_1", "chain_7"])
def test_small_robots(capi, kind):
    desc, ee, gr = small_robot(kind)
    h = capi.SolverHandle(desc, ee, gr, device=0)
    q = R.columns(desc, 3, 6)
    X = h.eval_points(0, q, [0.0, 0.0, 0.0], want=("xyz",))[0]
    paths = np.ascontiguousarray(q.T[None])
    all_pairs = ~np.eye(desc.n_links, dtype=bool)
    for M in (None, all_pairs, desc.self_pairs(), np.zeros_like(all_pairs)):
        h.set_self_pairs(M)
        d2, pair = R.reference_paths(X[None], desc.point_link, M)
        for c in (np.inf, 0.05):
            got = h.self_clearance(paths, cutoff=c)
            wd2, wpair = R.apply_cutoff(d2, pair, c)
            assert same(got["d2"], wd2) and same(got["pair"], wpair), (kind, c)
        if desc.n_links == 1 or not np.any(M if M is not None else all_pairs):
            assert np.isinf(d2).all() and (pair == -1).all()  # one link, or no pair: nothing to compare
    h.close()


# ---------------------------------------------------------------------------------------------- 4. non-finite columns
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_column_disturbs_no_other(rigs, bad):
    r = rigs("panda")
    r.h.set_self_pairs(r.masks["default"])
    d2, pair = r.want("default")
    paths, idx = r.paths(65, CHECK_TG + 2)
    spots = [(0, 1, 3), (1, 0, 0), (64, CHECK_TG + 1, 6), (64, 2, 2)]  # (path, column, joint)
    for b, t, j in spots:
        paths[b, j, t] = bad
    got = r.h.self_clearance(paths, cutoff=0.5)
    wd2, wpair = R.apply_cutoff(d2[idx], pair[idx], 0.5)
    for b, t, _ in spots:
        wd2[b, t], wpair[b, t] = np.nan, -1
    assert same(got["pair"], wpair)
    assert np.array_equal(np.isnan(got["d2"]), np.isnan(wd2)) and same(np.nan_to_num(got["d2"], nan=-1.0), np.nan_to_num(wd2, nan=-1.0))
    r.h.set_self_pairs(None)


# ---------------------------------------------------------------------------------------------- 5. host, device, busy stream
def test_device_entry_point_equals_the_host_one_also_behind_a_busy_stream(rigs):
    import time
    import torch
    r = rigs("fetch")
    r.h.set_self_pairs(r.masks["default"])
    paths, _ = r.paths(3, 9)
    c = 2 * r.clearance
    want = r.h.self_clearance(paths, cutoff=c)
    side = torch.cuda.Stream(device="cuda:0")
    with hs.Scenario() as sc:
        d_paths = sc.keep(cu(paths))
        d_d2 = sc.keep(torch.full((3, 9), -7.0, dtype=torch.float64, device="cuda:0"))
        d_pair = sc.keep(torch.full((3, 9, 2), -7, dtype=torch.int32, device="cuda:0"))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.h.self_clearance_device(3, 9, d_paths.data_ptr(), d_d2.data_ptr(), d_pair.data_ptr(), cutoff=c, stream=side.cuda_stream)
        t_host = time.perf_counter() - t0
        side.synchronize()
        assert same(d_d2.cpu().numpy(), want["d2"]) and same(d_pair.cpu().numpy(), want["pair"])
        # behind a hold: the call is entered and returns while the stream is busy (no synchronisation inside it), a look from
        # another stream under the same hold finds nothing written, and the same bits are there afterwards
        d_d2.fill_(-7.0), d_pair.fill_(-7)
        early_d2, early_pair = sc.keep(torch.zeros_like(d_d2)), sc.keep(torch.zeros_like(d_pair))
        probe = torch.cuda.Stream(device="cuda:0")
        torch.cuda.synchronize()
        event = hs.hold(side, hs.hold_ms(t_host))
        entered = hs.still_held(event)
        r.h.self_clearance_device(3, 9, d_paths.data_ptr(), d_d2.data_ptr(), d_pair.data_ptr(), cutoff=c, stream=side.cuda_stream)
        returned = hs.still_held(event)
        with torch.cuda.stream(probe):
            early_d2.copy_(d_d2, non_blocking=True), early_pair.copy_(d_pair, non_blocking=True)
        probe.synchronize()
        looked = hs.still_held(event)  # the look was over before the hold was
        side.synchronize()
        print(f"entered, returned, looked under the hold: {entered}, {returned}, {looked}; enqueue {1e3 * t_host:.3f} ms, "
              f"hold {hs.hold_ms(t_host):.0f} ms ({hs.method()})")
        assert entered and returned and looked
        assert (early_d2.cpu().numpy() == -7.0).all() and (early_pair.cpu().numpy() == -7).all()
        assert same(d_d2.cpu().numpy(), want["d2"]) and same(d_pair.cpu().numpy(), want["pair"])
    r.h.set_self_pairs(None)


def test_validation_and_the_empty_batch(rigs, capi):
    r = rigs("fetch")
    nd = r.desc.ndof
    empty = r.h.self_clearance(np.zeros((0, nd, 5)))
    assert empty["d2"].shape == (0, 5) and empty["pair"].shape == (0, 5, 2)
    for c in (0.0, -1.0, np.nan):
        with pytest.raises(capi.GTOError, match=r"failed \(-1\).*cutoff"):
            r.h.self_clearance(np.zeros((1, nd, 2)), cutoff=c)
    L = r.desc.n_links
    asym = np.zeros((L, L), dtype=bool)
    asym[0, 2] = True
    diag = np.eye(L, dtype=bool)
    r.h.set_self_pairs(r.masks["far"])
    before = r.h.self_clearance(np.ascontiguousarray(r.q.T[None]))
    for M, why in ((asym, "not symmetric"), (diag, "paired with itself")):
        with pytest.raises(capi.GTOError, match=why):
            r.h.set_self_pairs(M)
    after = r.h.self_clearance(np.ascontiguousarray(r.q.T[None]))  # a refused mask leaves the handle's mask alone
    assert same(before["d2"], after["d2"]) and same(before["pair"], after["pair"])
    r.h.set_self_pairs(None)


# ---------------------------------------------------------------------------------------------- 6. the Python layers
def test_chain_and_planner_report_the_calls_one_by_one(capi):
    import grasptrajopt_amd as g
    from grasptrajopt_amd import utils
    from grasptrajopt_amd.grasp_chain import GraspChain
    from test_gpu_grasp_chain import chain_setup
    B, n = 2, 3
    cfg, robot, fields, RT = chain_setup("panda", B * n, seed=21)
    RT = RT.reshape(B, n, 4, 4)
    qc = np.array(cfg["default_pose"], dtype=np.float64)
    base = np.array([0.01, -0.02, 0.0])
    chain = GraspChain(robot, cfg["link_ee"], cfg["link_gripper"])
    chain.max_iter = 20
    kw = dict(axis_standoff=cfg["axis_standoff"])
    lift = dict(mode="lift", distance=0.1, steps=4)
    spec = dict(q_ref=qc, cutoff=0.5)  # a wide cutoff: the plans' distances themselves, not "far"
    clearance, cutoff, mask = capi.self_check_request(robot.desc, spec)
    assert clearance == robot.desc.point_spacing() and cutoff == 0.5 and mask.sum() // 2 == 47
    assert capi.self_check_request(robot.desc, {})[1] == 2 * clearance
    plain = chain.plan_objects(qc, RT, RT, [n, n], fields[0], base, retrieve=dict(lift), self_check=None, **kw)
    got = chain.plan_objects(qc, RT, RT, [n, n], fields[0], base, retrieve=dict(lift), self_check=spec, **kw)
    added = ["retrieve_self_clear", "retrieve_self_d2", "retrieve_self_pair", "self_clear", "self_d2", "self_pair"]
    assert sorted(set(vars(got)) - set(vars(plain))) == added
    for k, v in vars(plain).items():  # self_check=None returns the old keys only, and every result there was is bit-equal
        assert same(v, getattr(got, k)), k
    h = chain._handle
    h.set_self_pairs(mask)
    for prefix, paths in (("self_", got.plans), ("retrieve_self_", got.retrieve_path)):
        one = h.self_clearance(paths, cutoff=cutoff)
        want = capi.self_check_summary(one["d2"], one["pair"], clearance, prefix)
        for k, v in want.items():
            assert same(getattr(got, k), v), k
        assert getattr(got, prefix + "d2").shape == (B,) and getattr(got, prefix + "pair").shape == (B, 2)
        print(prefix, "dist", np.sqrt(getattr(got, prefix + "d2")), "pair", getattr(got, prefix + "pair").tolist(),
              "clear", getattr(got, prefix + "clear").tolist())
    alone = chain.plan_objects(qc, RT, RT, [n, n], fields[0], base, self_check=spec, **kw)  # no retrieve: the plan's three only
    assert sorted(k for k in vars(alone) if "self_" in k) == added[3:] and same(alone.self_d2, got.self_d2)
    # the planner: one plan's retrieve path, and the per-waypoint dict of a plan
    planner = g.GTOPlanner(robot, cfg["link_ee"], cfg["link_gripper"])
    path, reached, checks = planner.retrieve_path(got.plans[1], "lift", distance=0.1, steps=4, self_check=spec)
    assert same(path, got.retrieve_path[1]) and sorted(checks) == ["self_clear", "self_d2", "self_pair"]
    for k, v in checks.items():
        assert same(np.asarray(v), getattr(got, "retrieve_" + k)[1]), k
    per = planner.self_clearance(got.plans, **spec)
    one = h.self_clearance(got.plans, cutoff=cutoff)
    assert same(per["d2"], one["d2"]) and same(per["pair"], one["pair"]) and same(per["clear"], one["dist"] >= clearance)
    assert same(utils.self_clearance(robot, got.plans[0], **spec)["d2"], one["d2"][0])
    chain.close()
    robot.close()
