"""GPU: the grasp collision filter on the stream -- gto_filter_grasps_device, SolverHandle.filter_grasps_device,
utils.filter_grasp_sets and GraspChain.plan_grasps -- against the numpy restatement (tests/grasp_filter_cases.py), the
existing kernel path Observation.check_posed, the reference's own counts (tests/golden/collision_checks.npz) and the
host-composed chain filter_grasp_sets -> GraspChain.plan_objects.  Every comparison is exact.  Run the file under a time
limit (timeout -k 10 900 pytest ...) and stop at the first fault."""
import numpy as np
import pytest

import cloud_cases as cc
import depth_cases as dc
import grasp_filter_cases as gf
import grasptrajopt_amd as g
from grasptrajopt_amd import synthetic as syn
from grasptrajopt_amd import utils
from conftest import golden
from helpers import cfg_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as gr
    gr.build()
    from grasptrajopt_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def handle(capi):
    cfg = cfg_of("panda")
    h = capi.SolverHandle(g.load_builtin("panda"), cfg["link_ee"], cfg["link_gripper"], device=0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def image_obs(capi):
    """The resident observation of an image of tests/depth_cases.py, built once."""
    from grasptrajopt_amd.observation import Observation
    made = {}

    def get(name):
        if name not in made:
            c = dc.cases()[name]
            made[name] = Observation.from_depth(c.depth, c.K, c.cam, c.mask, c.threshold)
        return made[name]
    yield get
    for o in made.values():
        o.close()


def cu(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")  # (a C-ordered copy: the cases' arrays are read-only)


OUTPUTS = ("counts", "keep", "kept_rows", "n_kept", "n_grasps", "plan_goals", "ik_goals")


def run_filter(h, inp, obs, skip=(), stream=None):
    """One call of the entry point on inputs `inp` (grasp_filter_cases) against the observations `obs`.  The outputs start at
    the restatement's sentinels (counts -1, keep 0, kept_rows -1, goals 0; the two per-object counts at -7), so what the
    kernels leave untouched compares too.  skip: outputs passed as NULL (they come back at their sentinels)."""
    import torch
    B, n_max = inp.grasps.shape[:2]
    f64, i32 = torch.float64, torch.int32
    dev = lambda shape, dt, fill: torch.full(shape, fill, dtype=dt, device="cuda:0")
    out = dict(counts=dev((B, n_max), i32, -1), keep=dev((B, n_max), torch.uint8, 0), kept_rows=dev((B, n_max), i32, -1),
               n_kept=dev((B,), i32, -7), n_grasps=dev((B,), i32, -7), plan_goals=dev((B, n_max, 4, 4), f64, 0.0),
               ik_goals=dev((B, n_max, 4, 4), f64, 0.0))
    keep_alive = [cu(inp.points), cu(inp.object_pose), cu(inp.grasps), cu(inp.n_grasps.astype(np.int32)),
                  None if inp.world_to_base is None else cu(inp.world_to_base), None if inp.base_pos is None else cu(inp.base_pos)]
    d_pts, d_op, d_gr, d_n, d_w, d_base = [None if t is None else t.data_ptr() for t in keep_alive]
    ptr = lambda k: None if k in skip else out[k].data_ptr()
    torch.cuda.synchronize()
    h.filter_grasps_device(obs, n_max, d_pts, len(inp.points), d_op, d_gr, d_n, inp.check_offset, inp.ik_offset, d_w, d_base,
                           inp.max_ratio, ptr("counts"), ptr("keep"), ptr("kept_rows"), ptr("n_kept"), ptr("n_grasps"),
                           ptr("plan_goals"), ptr("ik_goals"), stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_equals_restatement(got, want, what, skip=()):
    for k in ("counts", "keep", "kept_rows", "n_kept", "n_grasps"):
        if k not in skip:
            assert np.array_equal(got[k], getattr(want, k)), (what, k, got[k], getattr(want, k))
    for k in ("plan_goals", "ik_goals"):
        if k not in skip:
            assert gf.same_numbers(got[k], getattr(want, k)), (what, k)


# ---------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("name", gf.SWEEP_NAMES + gf.EDGE_NAMES)
def test_counts_goals_and_compaction_equal_the_restatement(handle, image_obs, name):
    inp = gf.sweep_case(name) if name in gf.SWEEP_NAMES else gf.edge_case(name)
    obs = [image_obs(i) for i in inp.images]
    got = run_filter(handle, inp, obs)
    want = inp.expected
    print(name, "draws", inp.draws, "counted rows", gf.row_counts(inp).tolist(), "kept", want.n_kept.tolist())
    assert_equals_restatement(got, want, name)
    # the counts against an independent, existing kernel path: Observation.check_posed at the host-composed poses
    for b, n in enumerate(gf.row_counts(inp)):
        C, _, _, bad = gf.compose(inp, b)
        posed = np.where(bad, -1, obs[b].check_posed(inp.points, C))
        assert np.array_equal(got["counts"][b, :n], posed), (name, b)


# ---------------------------------------------------------------------------------------------- 2. the reference's counts
def test_counts_equal_the_reference_run(handle):
    from grasptrajopt_amd.observation import Observation
    z = golden("collision_checks.npz")
    poses = np.asarray(z["poses"], dtype=np.float64).reshape(1, -1, 4, 4)
    n = poses.shape[1]
    inp = gf.SimpleNamespace(points=np.asarray(z["gripper_points"], dtype=np.float64), object_pose=np.eye(4)[None], grasps=poses,
                             n_grasps=np.array([n], np.int32), world_to_base=None, base_pos=None, check_offset=np.eye(4), ik_offset=None,
                             max_ratio=0.01)
    obs = Observation.from_depth(z["depth"], z["K"], z["cam"], z["mask"], float(z["threshold"]))
    got = run_filter(handle, inp, [obs])
    obs.close()
    want = np.asarray(z["grasp_counts"])
    assert np.array_equal(got["counts"][0], want)  # products with identities are exact
    keep = want / len(inp.points) <= 0.01
    assert np.array_equal(got["keep"][0].astype(bool), keep) and got["n_kept"][0] == keep.sum()
    assert np.array_equal(got["kept_rows"][0, :keep.sum()], np.flatnonzero(keep))
    assert got["plan_goals"][0, :keep.sum()].tobytes() == np.ascontiguousarray(poses[0, keep]).tobytes()


# ---------------------------------------------------------------------------------------------- 3. one observation per object
def test_every_object_is_tested_against_its_own_observation(handle, image_obs):
    inp = gf.sweep_case("p256_n65_b3")  # three objects, three different images
    assert len(set(inp.images)) == 3
    obs = [image_obs(i) for i in inp.images]
    big = run_filter(handle, inp, obs)
    assert_equals_restatement(big, inp.expected, "three images")
    for b in range(3):  # one call per object
        one = run_filter(handle, gf.select(inp, [b]), [obs[b]])
        for k in OUTPUTS:
            assert one[k].tobytes() == big[k][b:b + 1].tobytes(), (b, k)
    for order in ([2, 0, 1], [1, 1, 2, 1], [0, 0]):  # permuted; repeated entries of obs
        sub = gf.select(inp, order)
        got = run_filter(handle, sub, [obs[b] for b in order])
        assert_equals_restatement(got, sub.expected, order)
        for k in OUTPUTS:
            assert got[k].tobytes() == big[k][order].tobytes(), (order, k)


# ---------------------------------------------------------------------------------------------- 4. non-finite rows
def test_non_finite_rows_report_minus_one_and_change_nobody_else(handle, image_obs):
    inp = gf.edge_case("mixed")
    obs = [image_obs(i) for i in inp.images]
    got = run_filter(handle, inp, obs)
    assert_equals_restatement(got, inp.expected, "mixed")
    assert got["counts"][4].tolist() == [0, -1, -1, 0] and got["keep"][4].tolist() == [1, 0, 0, 1]
    clean = gf.SimpleNamespace(**vars(inp))
    clean.grasps = inp.grasps.copy()
    clean.grasps[4, 1:3] = inp.grasps[4, 0]
    ref = run_filter(handle, clean, obs)
    for k in OUTPUTS:  # the other objects, and the other rows of object 4
        assert np.delete(got[k], 4, axis=0).tobytes() == np.delete(ref[k], 4, axis=0).tobytes(), k
    assert got["counts"][4, [0, 3]].tolist() == ref["counts"][4, [0, 3]].tolist()
    assert gf.same_numbers(got["plan_goals"][4, :2], ref["plan_goals"][4, [0, 3]])
    # an object without a kept row: n_kept 0, n_grasps 1, position 0 = row 0's goals, kept_rows[0] = -1
    for name, b in (("mixed", 1), ("nan_object", 0), ("inf_world_to_base", 1)):
        c = gf.edge_case(name)
        r = run_filter(handle, c, [image_obs(i) for i in c.images])
        assert_equals_restatement(r, c.expected, name)
        _, A, ik, _ = gf.compose(c, b)
        assert (r["n_kept"][b], r["n_grasps"][b], r["kept_rows"][b, 0]) == (0, 1, -1) and not r["keep"][b].any()
        assert gf.same_numbers(r["plan_goals"][b, 0], A[0]) and gf.same_numbers(r["ik_goals"][b, 0], ik[0])
        assert not r["plan_goals"][b, 1:].any() and not r["ik_goals"][b, 1:].any()


# ---------------------------------------------------------------------------------------------- 5. cloud observations
def test_cloud_runs_around_a_depth_object_equal_check_posed(handle, image_obs):
    from grasptrajopt_amd.observation import Observation
    P, k = 65, 11
    ca, cb = (cc.cases()[n] for n in cc.POSED_CASES)
    pts, RTa = cc.posed_instance(ca, P)
    _, RTb = cc.posed_instance(cb, P)
    oa, ob = Observation.from_cloud(ca.points, ca.normals, k), Observation.from_cloud(cb.points, cb.normals, k)
    image = "pow2_over"  # a depth object in the middle, with the clouds' points
    n_max = 6
    rng = np.random.default_rng(17)
    im = dc.cases()[image]
    near = np.flatnonzero(np.abs(im.query).max(axis=1) < 1.0e5)
    RTd = np.stack([gf.rigid(rng, 0.0, 0.6) for _ in range(n_max)])
    RTd[:, :3, 3] = im.query[near[rng.integers(len(near), size=n_max)]]
    targets = np.stack([RTa, RTa[::-1], RTd, RTb, RTb[[3, 4, 5, 0, 1, 2]]])
    targets = np.where(np.isfinite(targets), targets, 0.25)  # (the NaN goes into the grasps below)
    inp = gf.inputs_for(targets, ["-"] * 5, pts, [6, 5, 6, 6, 4], rng, True, True, True, max_ratio=0.25)
    inp.grasps[0, 2, 1, 3] = np.nan
    obs = [oa, oa, image_obs(image), ob, ob]
    got = run_filter(handle, inp, obs)
    for b, n in enumerate(gf.row_counts(inp)):
        C, A, ik, bad = gf.compose(inp, b)
        posed = np.where(bad, -1, obs[b].check_posed(pts, C))  # the existing launch chain, object by object
        assert np.array_equal(got["counts"][b, :n], posed) and (got["counts"][b, n:] == -1).all(), b
        # keep, compaction and goals from those counts, by the stated rule
        keep = (posed >= 0) & (posed / np.float64(P) <= inp.max_ratio)
        rows = np.flatnonzero(keep)
        take = rows if len(rows) else np.array([0])
        assert np.array_equal(got["keep"][b, :n].astype(bool), keep) and got["n_kept"][b] == len(rows)
        assert got["n_grasps"][b] == max(len(rows), 1) and np.array_equal(got["kept_rows"][b, :len(rows)], rows)
        assert gf.same_numbers(got["plan_goals"][b, :len(take)], A[take]) and gf.same_numbers(got["ik_goals"][b, :len(take)], ik[take])
    assert got["counts"][0, 2] == -1 and (got["counts"][[0, 1, 3, 4]] > 0).any() and (got["n_kept"] > 0).any()
    oa.close()
    ob.close()


def test_a_cloud_run_takes_a_second_launch_chain(handle):
    """One object on a cloud observation with the instance of test_check_posed_takes_a_second_launch_chain: 4096 gripper points
    at 4097 poses are 2^24 + 4096 queries, so the run's poses 0..4095 go into the first launch chain (kCheckChunkQueries =
    2^24, gto_api.hip) and pose 4096 alone into a second.  Identity object pose and check_offset: the check pose is the grasp."""
    from grasptrajopt_amd.observation import Observation
    s = cc.CHUNK_POSED
    assert cc.CHUNK_QUERIES == 1 << 24 and cc.CHUNK_QUERIES // s.P == s.n - 1
    points, normals, pts, poses, _ = cc.chunk_posed_instance()
    inp = gf.SimpleNamespace(points=pts, object_pose=np.eye(4)[None], grasps=poses[None], n_grasps=np.array([s.n], np.int32),
                             world_to_base=None, base_pos=None, check_offset=np.eye(4), ik_offset=None, max_ratio=0.25)
    obs = Observation.from_cloud(points, normals, s.k)
    got = run_filter(handle, inp, [obs])
    C, A, ik, bad = gf.compose(inp, 0)
    posed = np.where(bad, -1, obs.check_posed(pts, C))
    obs.close()
    assert bad[2::6].all() and not np.delete(bad, np.arange(2, s.n, 6)).any()
    assert np.array_equal(got["counts"][0], posed) and 0 < posed[4096] < s.P
    keep = (posed >= 0) & (posed / np.float64(s.P) <= inp.max_ratio)
    rows = np.flatnonzero(keep)
    assert 0 < len(rows) < (~bad).sum()  # some finite rows are kept and some are not
    assert np.array_equal(got["keep"][0].astype(bool), keep) and got["n_kept"][0] == len(rows) == got["n_grasps"][0]
    assert np.array_equal(got["kept_rows"][0, :len(rows)], rows) and (got["kept_rows"][0, len(rows):] == -1).all()
    assert gf.same_numbers(got["plan_goals"][0, :len(rows)], A[rows]) and gf.same_numbers(got["ik_goals"][0, :len(rows)], ik[rows])


# ---------------------------------------------------------------------------------------------- 6. validation
def test_the_entry_point_validates_on_the_host(capi, handle, image_obs):
    import ctypes as C
    import torch
    lib = capi.load_library()
    o = image_obs("tile_plus_one")
    x = torch.zeros(4096, dtype=torch.float64, device="cuda:0").data_ptr()
    I = np.eye(4)
    ok = dict(observations=[o], n_max=1, points=x, P=1, object_pose=x, grasps=x, n_grasps=x, check_offset=I)
    handle.filter_grasps_device(**ok)  # every output NULL: nothing to write, and no fault
    handle.filter_grasps_device(**dict(ok, observations=[]))  # B = 0: GTO_OK without a launch
    handle.filter_grasps_device(**dict(ok, observations=[], points=None, grasps=None))
    torch.cuda.synchronize()
    bad = I.copy()
    bad[1, 2] = np.inf
    invalid = [dict(n_max=0), dict(P=0), dict(max_ratio=-0.5), dict(max_ratio=float("nan")), dict(max_ratio=float("inf")),
               dict(points=None), dict(object_pose=None), dict(grasps=None), dict(n_grasps=None), dict(check_offset=bad),
               dict(ik_offset=bad * np.nan)]
    for kw in invalid:
        with pytest.raises(capi.GTOError, match=r"\(-1\)"):
            handle.filter_grasps_device(**dict(ok, **kw))
    # what the wrapper cannot pass: B < 0, null obs, a null entry of obs, null check_offset, a null handle
    one, obs1 = (C.c_double * 16)(*I.ravel()), (C.c_void_p * 1)(o._ptr())
    null_entry = (C.c_void_p * 1)(None)
    v = C.c_void_p(x)
    raw = lambda h_, B, obs_, co: lib.gto_filter_grasps_device(h_, B, 1, obs_, v, 1, v, v, v, None, None, co, None, 0.01,
                                                             None, None, None, None, None, None, None, None)
    assert raw(handle._h, 1, obs1, one) == 0
    assert raw(handle._h, -1, obs1, one) == -1 and raw(handle._h, 1, None, one) == -1 and raw(handle._h, 1, null_entry, one) == -1
    assert raw(handle._h, 1, obs1, None) == -1 and raw(None, 1, obs1, one) == -1
    for kw in (dict(observations=[o] * 65536), dict(n_max=65536)):  # GTO_ERR_UNSUPPORTED
        with pytest.raises(capi.GTOError, match=r"\(-4\)"):
            handle.filter_grasps_device(**dict(ok, **kw))
    if torch.cuda.device_count() > 1:  # an observation on another device than the handle's
        from grasptrajopt_amd.observation import Observation
        c = dc.cases()["tile_plus_one"]
        far = Observation.from_depth(c.depth, c.K, c.cam, c.mask, c.threshold, device=1)
        with pytest.raises(capi.GTOError, match=r"\(-1\).*another device"):
            handle.filter_grasps_device(**dict(ok, observations=[far]))
        far.close()
    torch.cuda.synchronize()
    # an output set to NULL is skipped, the others are what they were
    inp = gf.edge_case("mixed")
    obs = [image_obs(i) for i in inp.images]
    full = run_filter(handle, inp, obs)
    for skip in (("counts", "keep"), ("kept_rows", "n_kept", "plan_goals"), ("n_grasps", "ik_goals")):
        got = run_filter(handle, inp, obs, skip=skip)
        assert_equals_restatement(got, inp.expected, skip, skip=skip)
        for k in OUTPUTS:
            if k not in skip:
                assert got[k].tobytes() == full[k].tobytes(), (skip, k)
    # it reads no kinematics: a handle with nine optimised joints, which the IK, seed and report entry points refuse
    from helpers import limit_robot
    desc, ee = limit_robot("chain", n_opt=9)
    hw = capi.SolverHandle(desc, ee, ee, device=0)
    assert_equals_restatement(run_filter(hw, inp, obs), inp.expected, "nine joints")
    hw.close()


# ---------------------------------------------------------------------------------------------- 7. the chain
def flat_image(depth_of):
    """A camera behind the robot looking along +x (synthetic.wall_scene's, at 60 x 80 pixels) whose image is depth_of(column)."""
    H, W = 60, 80
    K = np.array([[75.0, 0, 40.0], [0, 75.0, 30.0], [0, 0, 1.0]])
    cam = np.eye(4)
    cam[:3, :3] = np.array([[0, 0, 1.0], [-1.0, 0, 0], [0, -1.0, 0]])
    cam[:3, 3] = [-0.9, 0.0, 0.5]
    rng = np.random.default_rng(9)
    depth = (np.tile(depth_of(np.arange(W)), (H, 1)) + rng.uniform(-0.004, 0.004, (H, W))).astype(np.float32)
    return depth, K, cam


@pytest.fixture(scope="module")
def chain_case():
    from grasptrajopt_amd.grasp_chain import GraspChain
    from grasptrajopt_amd.observation import Observation
    B, n = 3, 8
    rng = np.random.default_rng(41)
    cfg = cfg_of("panda")
    robot = g.GTORobotModel(desc=g.load_builtin("panda"), time_derivs=[0, 1], param_joints=cfg["param_joints"],
                            collision_link_names=cfg["collision_link_names"], device=0)
    robot.setup_points_field(rng.uniform([0.25, -0.45, -0.02], [0.8, 0.45, 0.35], size=(400, 3)))
    wp = robot.workspace_points
    qd = np.abs(wp - np.array([0.6, 0.1, 0.1])) - np.array([0.06, 0.06, 0.1])
    d_box = np.linalg.norm(np.maximum(qd, 0), axis=1) + np.minimum(qd.max(axis=1), 0)
    fields = (syn.sdf_cost_map(np.minimum(wp[:, 2], d_box), epsilon=0.06).astype(np.float32),
              syn.sdf_cost_map(np.minimum(wp[:, 2], d_box + 0.03), epsilon=0.06).astype(np.float32))
    RT, _ = syn.make_goals(robot.desc, robot._util_handle().eval_fk, cfg["link_ee"], B * n, seed=41, ylim=(-0.3, 0.3), zlim=(0.15, 0.6))
    RT = RT.reshape(B, n, 4, 4)
    O = np.stack([gf.rigid(rng, 0.0, 0.8) for _ in range(B)])  # the object's pose: its grasps' centre, turned
    O[:, :3, 3] = RT[:, :, :3, 3].mean(axis=1)
    grasps = np.linalg.inv(O)[:, None] @ RT
    # object 0 stands behind a surface 0.5 m from the camera (no grasp free), object 1 in front of one 3 m away (every grasp
    # free), object 2 sees the near surface in the image's left half only
    images = [flat_image(lambda u: np.full(u.shape, 0.5)), flat_image(lambda u: np.full(u.shape, 3.0)),
              flat_image(lambda u: np.where(u < 40, 0.5, 3.0))]
    obs = [Observation.from_depth(d, K, cam, None, 4.0) for d, K, cam in images]
    chain = GraspChain(robot, cfg["link_ee"], cfg["link_gripper"], standoff_distance=-0.1, standoff_offset=-10)
    chain.max_iter, chain.ik_max_iter = 30, 20
    case = gf.SimpleNamespace(B=B, n=n, cfg=cfg, robot=robot, fields=fields, O=O, grasps=grasps, obs=obs, chain=chain,
                              qc=np.array(cfg["default_pose"], dtype=np.float64), base=np.array([0.01, -0.02, 0.0]),
                              points=rng.uniform(-0.04, 0.04, (100, 3)), check_offset=syn.standoff_pose(-0.03, cfg["axis_standoff"]),
                              ik_offset=syn.standoff_pose(-0.1, cfg["axis_standoff"]), n_grasps=np.array([8, 8, 7], np.int32))
    yield case
    chain.close()
    for o in obs:
        o.close()
    robot.close()


@pytest.mark.parametrize("n_seeds", [1, 2])
def test_plan_grasps_is_the_host_filter_followed_by_plan_objects(chain_case, n_seeds):
    c = chain_case
    kw = dict(axis_standoff=c.cfg["axis_standoff"], pos_tol=0.05, rot_tol_deg=360.0, ik_collision_threshold=1.0e9, n_seeds=n_seeds)
    if n_seeds > 1:
        kw["observation"] = c.obs[1]
    fs = utils.filter_grasp_sets(c.obs, c.points, c.O, c.grasps, c.n_grasps, c.check_offset, c.ik_offset, None, c.base)
    assert fs["n_kept"][0] == 0 and fs["n_kept"][1] == c.n and 0 < fs["n_kept"][2] < c.n_grasps[2]
    want = c.chain.plan_objects(c.qc, fs["ik_goals"], fs["plan_goals"], fs["n_grasps"], c.fields, c.base, **kw)
    got = c.chain.plan_grasps(c.qc, c.O, c.grasps, c.n_grasps, c.obs, c.fields, c.base, c.points, c.check_offset, ik_offset=c.ik_offset, **kw)
    assert np.array_equal(got.grasp_counts, fs["counts"]) and np.array_equal(got.grasp_keep, fs["keep"])
    assert np.array_equal(got.kept_rows, fs["kept_rows"]) and np.array_equal(got.n_kept, fs["n_kept"])
    for k in ("plans", "dQ", "cost", "iters", "status", "n_accepted", "seed_index", "q_solutions", "accept", "err_pos", "err_rot"):
        assert np.ascontiguousarray(getattr(got, k)).tobytes() == np.ascontiguousarray(getattr(want, k)).tobytes(), k
    assert (want.n_accepted[1:] > 0).all()  # grasp_row has rows to name
    rows = np.arange(c.B)
    if n_seeds == 1:
        pos = np.array([np.flatnonzero(want.accept[b, :fs["n_grasps"][b]])[want.seed_index[b]] if want.seed_index[b] >= 0 else -1
                        for b in rows])
    else:
        pos = want.goal_row
        assert np.array_equal(got.goal_row, want.goal_row) and np.array_equal(got.best_slot, want.best_slot)
    named = np.where((fs["n_kept"] > 0) & (want.n_accepted > 0) & (pos >= 0), fs["kept_rows"][rows, np.maximum(pos, 0)], -1)
    assert np.array_equal(got.grasp_row, named) and got.grasp_row[0] == -1 and (got.grasp_row[1:] >= 0).all()
    assert fs["keep"][rows[1:], got.grasp_row[1:]].all()  # an original row that was kept
