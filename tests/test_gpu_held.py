"""GPU: the held object's points in collision along the motion after the grasp -- gto_check_held_paths(_device),
Observation.check_held_paths, GTOPlanner.retrieve_path(held_points=...), GraspChain.plan_objects(retrieve={held_points...})
-- against the numpy restatement of tests/held_ref.py on the FP64 oracle's link_ee frames.  Every case is decided by a margin
of 1e-9 (tests/test_held_cpu.py), four orders above what gto_eval_fk is held to the oracle, so every comparison of counts is
exact.  Run the file under a time limit (timeout -k 10 600 pytest ...) and stop at the first fault."""
import time

import numpy as np
import pytest

import held_ref as hr
from helpers import exhaustive

pytestmark = pytest.mark.gpu

INVALID = r"\(-1\)"  # GTO_ERR_INVALID_ARG in a GTOError's text


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


def cu(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to("cuda:0")  # (a copy: the cases' arrays are read-only)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Setup:
    """A case of held_ref with its handle (horizon 12, standoff_offset -2: the reversed stretch is columns 10 .. 0) and its
    observations, built once per robot."""

    def __init__(self, capi, oracle_mod, name):
        from grasptrajopt_amd.observation import Observation
        self.s = s = hr.case(oracle_mod, name)
        self.h = capi.SolverHandle(s.desc, s.ee, s.gripper, oracle_mod.reference_opts(T=hr.TP_FULL, standoff_offset=-2), device=0,
                                   n_gripper_points=s.ngp)
        self.depth = Observation.from_depth(s.depth, s.K, s.cam, None, s.threshold)
        self.clouds = {k: Observation.from_cloud(s.points, s.normals, k) for k in hr.CLOUD_KS}
        self.want = {kind: hr.expected(oracle_mod, name, kind)[0] for kind in hr.KINDS}

    def obs(self, kind):
        return self.depth if kind in ("depth", "labels") else self.clouds[int(kind[5:])]

    def labels(self, kind):
        return dict(labels=self.s.labels, held_label=hr.LABEL_OBJECT) if kind == "labels" else {}

    def run(self, kind, Tp=hr.TP_FULL - 1, rows=slice(None), **kw):
        s = self.s
        args = dict(n_held=s.n_held[rows], base_pos=s.base)
        args.update(self.labels(kind))
        args.update(kw)
        return self.h.check_held_paths(self.obs(kind), s.paths[rows, :, :Tp], args.pop("held", s.held[rows]), **args)

    def close(self):
        self.h.close()
        self.depth.close()
        for o in self.clouds.values():
            o.close()


@pytest.fixture(scope="module")
def setups(capi, oracle_mod):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Setup(capi, oracle_mod, name)
        return made[name]

    yield get
    for v in made.values():
        v.close()


# ---------------------------------------------------------------------------------------------- 1. counts, Tp, TG, batches
@pytest.mark.parametrize("name", hr.ROBOTS)
def test_counts_equal_the_restatement_at_every_length(setups, name):
    c = setups(name)
    for kind in hr.KINDS:
        for Tp in hr.TPS:
            got = c.run(kind, Tp)
            assert got.dtype == np.int32
            np.testing.assert_array_equal(got, c.want[kind][:, :Tp], err_msg=f"{kind}, Tp = {Tp}")
        if kind.startswith("cloud"):
            with exhaustive():
                np.testing.assert_array_equal(c.run(kind), c.want[kind][:, :hr.TP_FULL - 1], err_msg=f"{kind}, exhaustive")
    assert (c.want["labels"] != c.want["depth"]).any()  # the rule was felt


@pytest.mark.parametrize("name", hr.ROBOTS)
def test_counts_do_not_depend_on_the_columns_per_workgroup(setups, monkeypatch, name):
    c = setups(name)
    for tg in ("1", "2", "3", "4"):
        monkeypatch.setenv("GTO_CHECK_TG", tg)
        for kind in ("labels", "cloud11"):
            for Tp in (5, 11):
                np.testing.assert_array_equal(c.run(kind, Tp), c.want[kind][:, :Tp], err_msg=f"GTO_CHECK_TG={tg}, {kind}, Tp = {Tp}")
    monkeypatch.delenv("GTO_CHECK_TG")


@pytest.mark.parametrize("name", ["panda", "chain16"])
def test_a_plan_alone_gives_the_batch_rows_bits(setups, name):
    c = setups(name)
    for kind in ("depth", "labels", "cloud1", "cloud11"):
        batch = c.run(kind)
        for b in range(hr.B):
            assert same(c.run(kind, rows=slice(b, b + 1)), batch[b:b + 1]), (kind, b)
        back = c.run(kind, rows=slice(None, None, -1))  # every plan at another position
        assert same(back[::-1], batch), kind


# ---------------------------------------------------------------------------------------------- 2. attach
@pytest.mark.parametrize("name", hr.ROBOTS)
def test_attach_null_is_column_0_and_the_reverse_mode_names_the_plans_last_column(setups, name):
    import torch
    c, s = setups(name), setups(name).s
    for kind in ("labels", "cloud11"):
        lift = c.run(kind)
        assert same(c.run(kind, attach=s.paths[:, :, :hr.TP_FULL - 1], attach_col=0), lift), kind
        # the reversed stretch leaves the grasp column out: columns 1 .. 11 against the plans' last column
        rev = c.h.check_held_paths(c.obs(kind), s.paths[:, :, 1:], s.held, n_held=s.n_held, attach=s.reverse_plans, base_pos=s.base,
                                   **c.labels(kind))
        np.testing.assert_array_equal(rev, c.want[kind][:, 1:], err_msg=kind)
        wrong = c.h.check_held_paths(c.obs(kind), s.paths[:, :, 1:], s.held, n_held=s.n_held, base_pos=s.base, **c.labels(kind))
        assert not np.array_equal(wrong, rev), "a path that leaves the grasp out needs its attach column"
    # with the reverse kernel's own path, on the stream
    n = c.h.retrieve_path_columns()
    assert n == hr.TP_FULL - 1
    d_plans, d_path = cu(s.reverse_plans), torch.empty((hr.B, s.desc.ndof, n), dtype=torch.float64, device="cuda:0")
    d_held, d_n = cu(s.held), cu(s.n_held)
    d_lab, d_hl = cu(s.labels), cu(np.full(hr.B, hr.LABEL_OBJECT, np.int32))
    d_count = torch.full((hr.B, n), -7, dtype=torch.int32, device="cuda:0")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    c.h.retrieve_reverse(hr.B, d_plans.data_ptr(), [], 0.0, d_path.data_ptr(), stream=st.cuda_stream)
    c.h.check_held_paths_device(c.depth, hr.B, n, d_path.data_ptr(), d_held.data_ptr(), hr.P_MAX, d_n.data_ptr(), d_count.data_ptr(),
                                attach=d_plans.data_ptr(), attach_ld=hr.TP_FULL, attach_col=hr.TP_FULL - 1, labels=d_lab.data_ptr(),
                                held_label=d_hl.data_ptr(), base_pos=s.base, stream=st.cuda_stream)
    st.synchronize()
    assert same(d_path.cpu().numpy(), s.paths[:, :, 1:])
    np.testing.assert_array_equal(d_count.cpu().numpy(), c.want["labels"][:, 1:])


# ---------------------------------------------------------------------------------------------- 3. frames
@pytest.mark.parametrize("name", hr.ROBOTS)
def test_object_frame_points_with_the_objects_pose(setups, oracle_mod, name):
    c, s = setups(name), setups(name).s
    for kind in hr.KINDS:
        want = hr.expected(oracle_mod, name, kind, "object")[0]
        got = c.run(kind, held=s.held_obj, object_pose=s.pose)
        np.testing.assert_array_equal(got, want[:, :hr.TP_FULL - 1], err_msg=kind)
        np.testing.assert_array_equal(got, c.run(kind), err_msg=f"{kind}: the same points in the world frame")
    lists = [s.held[b, :n] for b, n in enumerate(hr.N_HELD)]  # a list of per-plan arrays in place of the padded array
    assert same(c.depth.check_held_paths(c.h, s.paths, lists, base_pos=s.base), c.run("depth", hr.TP_FULL))


# ---------------------------------------------------------------------------------------------- 4. non-finite inputs
@pytest.mark.parametrize("name", ["panda", "bushy8"])
@pytest.mark.parametrize("kind", ["labels", "cloud11"])
def test_non_finite_inputs_change_what_the_contract_names(setups, oracle_mod, name, kind):
    c, s = setups(name), setups(name).s
    Tp = hr.TP_FULL - 1
    clean = c.want[kind][:, :Tp]
    j = int(s.desc.opt_index[len(s.desc.opt_index) // 2])
    others = lambda b: np.arange(hr.B) != b
    # a column
    paths = s.paths[:, :, :Tp].copy()
    paths[5, j, 3] = np.nan
    got = c.h.check_held_paths(c.obs(kind), paths, s.held, n_held=s.n_held, base_pos=s.base, **c.labels(kind))
    want = clean.copy()
    want[5, 3] = -1
    np.testing.assert_array_equal(got, want, err_msg="a NaN path column")
    # q_att: column 0 of the path (attach NULL), and an attach array of its own
    paths = s.paths[:, :, :Tp].copy()
    paths[3, j, 0] = np.inf
    got = c.h.check_held_paths(c.obs(kind), paths, s.held, n_held=s.n_held, base_pos=s.base, **c.labels(kind))
    assert (got[3] == -1).all() and same(got[others(3)], clean[others(3)]), "a non-finite q_att in the path's column 0"
    att = s.reverse_plans.copy()
    att[3, j, -1] = np.nan
    att[2, j, 4] = np.nan  # (a column nobody reads)
    got = c.h.check_held_paths(c.obs(kind), s.paths[:, :, 1:], s.held, n_held=s.n_held, attach=att, base_pos=s.base, **c.labels(kind))
    assert (got[3] == -1).all() and same(got[others(3)], c.want[kind][:, 1:][others(3)]), "a NaN q_att in attach"
    # the base
    bases = np.tile(s.base, (hr.B, 1))
    assert same(c.run(kind, base_pos=bases), clean)  # per-plan bases that are all the shared one: the same bits
    bases[6, 2] = np.nan
    got = c.run(kind, base_pos=bases)
    assert (got[6] == -1).all() and same(got[others(6)], clean[others(6)]), "a NaN base"
    # the object's pose
    pose = s.pose.copy()
    pose[4, 1, 3] = np.nan
    got = c.run(kind, held=s.held_obj, object_pose=pose)
    assert (got[4] == -1).all() and same(got[others(4)], clean[others(4)]), "a NaN object pose"
    # one held point
    b, i = hr.NAN_POINT
    held = s.held.copy()
    held[b, i, 1] = np.nan
    want = hr.expected(oracle_mod, name, kind, nan_point=True)[0][:, :Tp]
    np.testing.assert_array_equal(c.run(kind, held=held), want, err_msg="a NaN held point")
    assert same(want[others(b)], clean[others(b)])
    plain = c.run("depth", held=held)  # without labels every point counts at the grasp column: now one less
    assert plain[b, 0] == hr.N_HELD[b] - 1 and same(plain[others(b)], c.want["depth"][:, :Tp][others(b)])
    held[b, i] = [np.inf, 0.0, -np.inf]
    np.testing.assert_array_equal(c.run(kind, held=held), want, err_msg="an infinite held point")


# ---------------------------------------------------------------------------------------------- 5. the device variant
@pytest.mark.parametrize("name", ["panda", "chain16"])
def test_device_variant_on_a_side_stream_and_clamped_counts(setups, capi, name):
    import torch
    c, s = setups(name), setups(name).s
    Tp = hr.TP_FULL - 1
    side = torch.cuda.Stream(device="cuda:0")
    d_paths, d_held, d_pose, d_obj = cu(s.paths[:, :, :Tp]), cu(s.held), cu(s.pose.reshape(hr.B, 16)), cu(s.held_obj)
    d_lab, d_hl = cu(s.labels), cu(np.full(hr.B, hr.LABEL_OBJECT, np.int32))
    wild = s.n_held.copy()
    wild[0], wild[6] = -5, 999  # read as 0 and as P_max
    for n_held in (s.n_held, wild):
        d_n = cu(n_held)
        for kind in hr.KINDS:
            d_count = torch.full((hr.B, Tp), -7, dtype=torch.int32, device="cuda:0")
            kw = dict(labels=d_lab.data_ptr(), held_label=d_hl.data_ptr()) if kind == "labels" else {}
            torch.cuda.synchronize()
            c.h.check_held_paths_device(c.obs(kind), hr.B, Tp, d_paths.data_ptr(), d_held.data_ptr(), hr.P_MAX, d_n.data_ptr(),
                                        d_count.data_ptr(), base_pos=s.base, stream=side.cuda_stream, **kw)
            side.synchronize()
            assert same(d_count.cpu().numpy(), c.run(kind)), kind
    d_count = torch.full((hr.B, Tp), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    c.h.check_held_paths_device(c.depth, hr.B, Tp, d_paths.data_ptr(), d_obj.data_ptr(), hr.P_MAX, cu(s.n_held).data_ptr(),
                                d_count.data_ptr(), object_pose=d_pose.data_ptr(), base_pos=s.base, stream=side.cuda_stream)
    side.synchronize()
    assert same(d_count.cpu().numpy(), c.run("depth", held=s.held_obj, object_pose=s.pose))
    for bad in (-1, hr.P_MAX + 1):  # the host variant sees the counts: a value outside [0, P_max] fails the call
        n_held = s.n_held.copy()
        n_held[2] = bad
        with pytest.raises(capi.GTOError, match=INVALID):
            c.run("depth", n_held=n_held)


# ---------------------------------------------------------------------------------------------- 6. the second launch chain
def test_a_cloud_check_takes_a_second_launch_chain(capi, oracle_mod):
    """chain16, Tp = 65, P_max = 4096, B = 64: chunk_items(64, 65 * 4096) = 63 plans go into the first launch chain and plan 63,
    the only one that holds all 4096 points, alone into a second."""
    from grasptrajopt_amd.observation import Observation
    k = hr.chunk_instance(oracle_mod)
    h = capi.SolverHandle(k.desc, k.ee, k.gripper, oracle_mod.reference_opts(), device=0, n_gripper_points=k.ngp)
    obs = Observation.from_cloud(k.points, k.normals, hr.CHUNK.k)
    t0 = time.perf_counter()
    got = h.check_held_paths(obs, k.paths, k.held, n_held=k.n_held, base_pos=k.base)
    print(f"check_held_paths, {hr.CHUNK.B} plans x {hr.CHUNK.Tp} columns x {hr.CHUNK.P_max} rows: {1e3 * (time.perf_counter() - t0):.1f} ms")
    np.testing.assert_array_equal(got, k.counts)
    obs.close()
    h.close()


# ---------------------------------------------------------------------------------------------- 7. errors
def test_the_entry_points_validate_on_the_host(setups, capi):
    import ctypes as C
    import torch
    from grasptrajopt_amd.observation import Observation
    c, s = setups("panda"), setups("panda").s
    h, lib = c.h, c.h.lib
    Tp = 4
    paths = np.ascontiguousarray(s.paths[:, :, :Tp])
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    labels, hl = np.ascontiguousarray(s.labels), np.full(hr.B, hr.LABEL_OBJECT, np.int32)
    count = np.full((hr.B, Tp), -7, np.int32)
    held, n_held, base = np.ascontiguousarray(s.held), np.ascontiguousarray(s.n_held), np.ascontiguousarray(s.base)

    def host(handle=h._h, obs=c.depth._ptr(), B=hr.B, Tp=Tp, paths=paths, attach=None, ld=0, col=0, held=held, P_max=hr.P_MAX,
             n_held=n_held, pose=None, labels=None, hl=None, base=base, count=count):
        return lib.gto_check_held_paths(handle, obs, B, Tp, ptr(paths, pd), ptr(attach, pd), ld, col, ptr(held, pd), P_max, ptr(n_held, pi),
                                        ptr(pose, pd), ptr(labels, pi), ptr(hl, pi), ptr(base, pd), 0, ptr(count, pi))

    keep = dict(paths=cu(paths), held=cu(held), n_held=cu(n_held), count=cu(count), attach=cu(s.reverse_plans), labels=cu(labels))

    def device(**kw):
        d = dict(handle=h._h, obs=c.depth._ptr(), B=hr.B, Tp=Tp, paths=keep["paths"].data_ptr(), attach=None, ld=0, col=0,
                 held=keep["held"].data_ptr(), P_max=hr.P_MAX, n_held=keep["n_held"].data_ptr(), pose=None, labels=None, hl=None,
                 base=base, count=keep["count"].data_ptr())
        d.update(kw)
        vp = lambda v: None if v is None else C.c_void_p(v)
        return lib.gto_check_held_paths_device(d["handle"], d["obs"], d["B"], d["Tp"], vp(d["paths"]), vp(d["attach"]), d["ld"], d["col"],
                                               vp(d["held"]), d["P_max"], vp(d["n_held"]), vp(d["pose"]), vp(d["labels"]), vp(d["hl"]),
                                               ptr(d["base"], pd), 0, vp(d["count"]), None)

    assert host() == 0 and (count >= 0).all()
    att = np.ascontiguousarray(s.reverse_plans)
    for call in (host, device):  # the device variant validates host-side facts only: it returns before any pointer is read
        assert call(handle=None) == -1 and call(obs=None) == -1 and call(base=None) == -1
        assert call(B=-1) == -1 and call(Tp=0) == -1 and call(P_max=0) == -1
        assert call(paths=None) == -1 and call(held=None) == -1 and call(n_held=None) == -1 and call(count=None) == -1
        assert call(B=65536) == -4 and call(P_max=65536) == -4
        assert call(B=0) == 0 and call(B=0, paths=None, held=None, n_held=None, count=None) == 0  # no launch
    for col in (-1, hr.TP_FULL, hr.TP_FULL + 5):
        assert host(attach=att, ld=hr.TP_FULL, col=col) == -1 and device(attach=keep["attach"].data_ptr(), ld=hr.TP_FULL, col=col) == -1
    assert host(attach=att, ld=hr.TP_FULL, col=hr.TP_FULL - 1) == 0
    assert host(labels=labels, hl=None) == -1 and device(labels=keep["labels"].data_ptr(), hl=None) == -1
    assert host(obs=c.clouds[11]._ptr(), labels=labels, hl=None) == -1   # the pair is checked for either kind
    before = count.copy()
    assert host(obs=c.clouds[11]._ptr()) == 0
    cloud = count.copy()
    assert host(obs=c.clouds[11]._ptr(), labels=labels, hl=hl) == 0 and same(count, cloud)  # and ignored for a cloud
    assert host(labels=labels, hl=hl) == 0 and not same(count, before)
    assert host(attach=att, ld=3, col=3) == -1 and "attach_col" in lib.gto_last_error(h._h).decode()  # errors name their cause
    with pytest.raises(capi.GTOError, match="one point set and one count per path"):
        h.check_held_paths(c.depth, paths, s.held[:3], n_held=s.n_held[:3])
    with pytest.raises(capi.GTOError, match="attach must have shape"):
        h.check_held_paths(c.depth, paths, s.held, n_held=s.n_held, attach=s.reverse_plans[:2])
    if torch.cuda.device_count() > 1:
        other = Observation.from_depth(s.depth, s.K, s.cam, None, s.threshold, device=1)
        with pytest.raises(capi.GTOError, match="another device"):
            h.check_held_paths(other, paths, s.held, n_held=s.n_held)
        other.close()


# ---------------------------------------------------------------------------------------------- 8. the Python layers
@pytest.mark.parametrize("n_seeds", [1, 2])
def test_chain_and_planner_report_the_held_counts_of_a_direct_call(n_seeds):
    import grasptrajopt_amd as g
    from grasptrajopt_amd import synthetic as syn
    from grasptrajopt_amd.grasp_chain import GraspChain
    from test_gpu_grasp_chain import chain_setup
    B, n = 2, 3
    cfg, robot, fields, RT = chain_setup("panda", B * n, seed=21)
    RT = RT.reshape(B, n, 4, 4)
    qc = np.array(cfg["default_pose"], dtype=np.float64)
    base = np.array([0.01, -0.02, 0.0])
    chain = GraspChain(robot, cfg["link_ee"], cfg["link_gripper"])
    chain.max_iter = 20
    depth, Kc, cam, mask = syn.wall_scene()
    obs = g.DepthPointCloud(depth, Kc, cam, target_mask=mask, threshold=1.5).observation()
    rng = np.random.default_rng(3)
    held = [RT[b, 0, :3, 3] + base + rng.uniform(-0.06, 0.06, (m, 3)) for b, m in enumerate((70, 33))]
    labels = np.where(np.asarray(mask) != 0, 5, 0).astype(np.int32)
    kw = dict(axis_standoff=cfg["axis_standoff"], n_seeds=n_seeds, observation=obs)
    h = chain._handle
    for mode in (dict(mode="lift", distance=0.1, steps=4), dict(mode="reverse")):
        plain = chain.plan_objects(qc, RT, RT, [n, n], fields[0], base, retrieve=dict(mode), **kw)
        got = chain.plan_objects(qc, RT, RT, [n, n], fields[0], base, retrieve=dict(mode, held_points=held), **kw)
        assert sorted(set(vars(got)) - set(vars(plain))) == ["retrieve_held_counts"]
        for k, v in vars(plain).items():  # every result there was is bit-equal
            assert same(v, getattr(got, k)), k
        attach = None if mode["mode"] == "lift" else got.plans
        want = h.check_held_paths(obs, got.retrieve_path, held, attach=attach, base_pos=base)
        assert got.retrieve_held_counts.shape == got.retrieve_counts.shape and same(got.retrieve_held_counts, want)
        print(mode["mode"], "held counts", got.retrieve_held_counts.tolist())
        # the padded form with counts, labels and one label for all
        pts, cnt = h.pad_held_points(held)
        ruled = chain.plan_objects(qc, RT, RT, [n, n], fields[0], base,
                                   retrieve=dict(mode, held_points=pts, held_counts=cnt, labels=labels, held_label=5), **kw)
        assert same(ruled.retrieve_held_counts, h.check_held_paths(obs, got.retrieve_path, pts, n_held=cnt, attach=attach, labels=labels,
                                                                   held_label=5, base_pos=base))
        assert same(ruled.retrieve_path, got.retrieve_path)
        # GTOPlanner.retrieve_path for one plan: the same path as without held points, and the chain's counts
        planner = g.GTOPlanner(robot, cfg["link_ee"], cfg["link_gripper"])
        args = dict(distance=0.1, steps=4) if mode["mode"] == "lift" else {}
        path0, reached0 = planner.retrieve_path(got.plans[1], mode["mode"], **args)
        path, reached, checks = planner.retrieve_path(got.plans[1], mode["mode"], observation=obs, held_points=held[1], base_position=base,
                                                      **args)
        assert same(path, path0) and reached == reached0 and same(path, got.retrieve_path[1])
        assert sorted(checks) == ["held_counts"] and same(checks["held_counts"], got.retrieve_held_counts[1])
    with pytest.raises(TypeError, match="unexpected key"):
        chain.retrieve_spec(dict(held=held))
    chain.close()
    robot.close()


from test_gpu_grasp_filter import chain_case  # noqa: E402,F401  (the fixture of the grasp filter's chain test)


def test_plan_grasps_places_object_frame_points_at_its_object_poses(chain_case):
    c = chain_case
    rng = np.random.default_rng(12)
    held_obj = [rng.uniform(-0.05, 0.05, (m, 3)) for m in (40, 65, 9)]  # in each object's frame, around its origin
    kw = dict(axis_standoff=c.cfg["axis_standoff"], pos_tol=0.05, rot_tol_deg=360.0, ik_collision_threshold=1.0e9, observation=c.obs[2])
    args = (c.qc, c.O, c.grasps, c.n_grasps, c.obs, c.fields, c.base, c.points, c.check_offset)
    lift = dict(mode="lift", distance=0.1, steps=4)
    plain = c.chain.plan_grasps(*args, ik_offset=c.ik_offset, retrieve=dict(lift), **kw)
    got = c.chain.plan_grasps(*args, ik_offset=c.ik_offset, retrieve=dict(lift, held_points=held_obj), **kw)
    for k, v in vars(plain).items():
        assert same(v, getattr(got, k)), k
    want = c.chain._handle.check_held_paths(c.obs[2], got.retrieve_path, held_obj, object_pose=c.O, base_pos=c.base)
    assert same(got.retrieve_held_counts, want) and (want >= 0).all()
    print("held counts", want.tolist())
