"""GPU: the broad phase of every collision consumer against the FP64 oracle, which culls nothing, on sparse fields whose only
non-zero voxels sit on the edges of the culling rule (tests/cull_fields.py): exactly R index steps from a chunk centre's voxel
(kept at margin 0, culled at margin -1), gradient-only records, diagonal near misses (exact zeros on both sides), radii
around the distance field's cap, anisotropic, one-voxel-thin, coarse and far-away grids, and voxels only one field holds
on either side of the standoff waypoint.  Consumers: k_obstacle_gram (eval_obstacle_normal_eq and the solve), the step
kernel's prebroad_tail (more than GTO_FEW_INSTANCES instances in flight), k_ik_solve (the obstacle half only), the two
constructions of the distance field, and scenes shared by halves.

A build with -DGTO_BROAD_MARGIN=-1 shows the cases are sharp: each consumer family disagrees with the oracle there.

Tolerances are those of tests/test_gpu_parity.py: blocks 1e-8 relative, sums of squares 1e-11, trajectories 1e-6 rad after
the same iteration counts, costs 1e-8 relative."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cull_fields as cf
from grasptrajopt_amd import synthetic as syn
from grasptrajopt_amd.robot_desc import load_builtin
from helpers import cfg_of, random_robot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
VARIANTS = {}  # case -> kernel variants that ran (printed at the end of the module: pytest -s)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    yield _capi
    if VARIANTS:
        print("\nkernel variants reached:\n" + "\n".join(f"  {k}: {v}" for k, v in sorted(VARIANTS.items())))


def _ran(prof):
    return sorted(k for k, v in prof.items() if v[1] > 0)


# ------------------------------------------------------------------------------------------ problems
def moving_links(desc):
    """Links moved by an optimised joint (the others are static: accounted once, in the static-only pass)."""
    opt_frames = {f for f in range(desc.n_frames) if desc.q_index[f] in set(desc.opt_index.tolist())}
    out = []
    for l, f in enumerate(desc.link_frame):
        f, mv = int(f), False
        while f >= 0:
            mv |= f in opt_frames
            f = int(desc.parent[f])
        if mv:
            out.append(l)
    return out


class Setup:
    """A robot with one chunk per link, a batch of seeds, a handle and an oracle with the same options."""

    def __init__(self, om, robot, B, T, off, max_iter=3, seed=0, base=(0.0, 0.0, 0.0), cap_res=None):
        ngp = None
        if robot in ("panda", "fetch"):
            self.desc = cf.thin_robot(load_builtin(robot), seed=seed)
            cfg = cfg_of(robot)
            self.ee, gr = cfg["link_ee"], cfg["link_gripper"]
        else:  # "wide<n_opt>": a random tree with nine to sixteen optimised joints
            n_opt = int(robot[4:])
            desc, self.ee = random_robot(50 + n_opt, n_frames=max(n_opt + 4, 14), n_opt=n_opt)
            self.desc, gr, ngp = cf.thin_robot(desc, seed=seed), self.ee, 40
        self.moving = moving_links(self.desc)
        if cap_res is not None:  # three moving links scaled to 46.5, 47.5 and 48.5 voxels: R = 47, 48, 49 around the cap
            self.cap_res, self.cap_links = cap_res, self.moving[1:4]
            self.desc = cf.scale_links(self.desc, {l: (46.5 + i) * cap_res for i, l in enumerate(self.cap_links)})
        d = self.desc
        self.opts_kw = dict(T=T, standoff_offset=off, max_iter=max_iter)
        self.gr, self.ngp = gr, ngp
        self.o = om.Oracle(d, self.ee, gr, om.reference_opts(**self.opts_kw), n_gripper_points=ngp)
        self.geo_o = om.Oracle(d, self.ee, gr, om.reference_opts(**self.opts_kw), n_gripper_points=ngp)
        rng = np.random.default_rng(1000 + seed)
        if robot in ("panda", "fetch"):
            pose = np.array(cfg_of(robot)["default_pose"], dtype=np.float64)
            pose = np.concatenate([np.zeros(d.ndof - len(pose)), pose])
            qc = np.tile(pose, (B, 1))
        else:
            qc = rng.uniform(0.3 * d.lower, 0.3 * d.upper, size=(B, d.ndof))
        qg = rng.uniform(0.7 * d.lower, 0.7 * d.upper, size=(B, d.ndof))
        qg[:, d.param_index] = qc[:, d.param_index]
        self.qc, self.qg, self.B, self.T, self.ts = qc, qg, B, T, T + off
        self.goals = self.o.eval_fk(qg)[:, d.frame_index(self.ee)].reshape(B, 1, 16)
        self.S = syn.standoff_pose(-0.05, "z")
        self.base = np.tile(np.asarray(base, dtype=np.float64), (B, 1))
        self.Q0 = np.stack([syn.make_seed(qc[b], qg[b], T, d.param_index) for b in range(B)])

    def handle(self, capi, om, **kw):
        opts = om.reference_opts(**dict(self.opts_kw, **kw))
        h = capi.SolverHandle(self.desc, self.ee, self.gr, opts, device=0, n_gripper_points=self.ngp)
        h.set_mode(0)
        return h

    def box(self, Q=None):
        """World bounding box of the surface points over the seeds."""
        Q = self.Q0 if Q is None else Q
        qs = Q.transpose(0, 2, 1).reshape(-1, self.desc.ndof)
        xyz, _, _, _ = self.geo_o.eval_points(0, qs, np.repeat(self.base, Q.shape[2], axis=0), want_field=False)
        return xyz.reshape(-1, 3).min(axis=0), xyz.reshape(-1, 3).max(axis=0)

    def solve_args(self):
        return (0, self.qc, self.goals, 1, self.S, self.base, self.Q0)


def grid_maker(st, res, shape=None, pad=0.15, anchor=None, Q=None):
    """make(shift) -> Geometry over a grid of resolution res around the seeds' points (shape: fixed, centred on them;
    anchor: a corner of the box the grid is pinned to, so that most of the robot lies outside)."""
    lo, hi = st.box(Q)
    res = float(res)
    if shape is None:
        shape = tuple(int(x) for x in np.ceil((hi - lo + 2 * pad) / res))
        org = lo - pad
    else:
        ext = np.asarray(shape) * res
        org = 0.5 * (lo + hi) - 0.5 * ext
        if anchor is not None:
            org = np.where(np.asarray(anchor) > 0, hi - ext + 0.02, np.where(np.asarray(anchor) < 0, lo - 0.02, org))
    Q = st.Q0 if Q is None else Q

    def make(shift):
        return cf.Geometry(st.geo_o, st.desc, Q, st.base, cf.Grid(tuple(shape), tuple(org + shift * res), res))
    return make


def family_fields(st, family, seed=0):
    """FieldBuilder of one family on the setup's seeds."""
    w2 = lambda kind, **k: [dict(kind=kind, bs=[b], **k) for b in range(min(2, st.B))]
    gl = dict(links=st.moving)  # a static link's gradient record contributes nothing (its J is zero)
    if family == "edge":  # two axes at R: the finest resolution of these that offers such a point
        for res in (0.06, 0.1, 0.15, 0.3):
            try:
                return cf.search(grid_maker(st, res), st.ts, w2("edge"), seed=seed)
            except RuntimeError:
                pass
        raise RuntimeError("no edge design")
    if family == "gradient":
        return cf.search(grid_maker(st, 0.04), st.ts, w2("gradient", **gl), seed=seed)
    if family == "near":
        return cf.search(grid_maker(st, 0.04), st.ts, w2("near"), seed=seed)
    if family == "cap":  # (Setup(cap_res=...): links of R = 47, 48, 49) a grid around the R = 47 chunk at one waypoint
        l, res = st.cap_links[0], st.cap_res
        V = st.geo_o.eval_visual_tf(st.Q0[0, :, st.T // 2])[0, l]
        c = V[:3, :3] @ cf.chunk_spheres(st.desc)[0][l] + V[:3, 3] + st.base[0]
        make = lambda shift: cf.Geometry(st.geo_o, st.desc, st.Q0, st.base, cf.Grid((128, 128, 128), tuple(c - 64 * res + shift * res), res))
        return cf.search(make, st.ts,
                         [dict(kind="farthest", links=[l], bs=[0], ts=[st.T // 2])], seed=seed, shifts=24)
    if family.startswith("aniso"):
        shape = {"aniso1": (1, 40, 33), "aniso2": (3, 97, 50), "aniso3": (64, 2, 5)}[family]
        res = {"aniso1": 0.05, "aniso2": 0.025, "aniso3": 0.04}[family]
        return cf.search(grid_maker(st, res, shape=shape), st.ts, w2("gradient", **gl), seed=seed, shifts=24)
    if family == "face":  # a small grid in a corner of the robot's box: most chunk centres clip onto its faces
        return cf.search(grid_maker(st, 0.04, shape=(12, 12, 12), anchor=(1, -1, 1)), st.ts, w2("gradient", outside=True, **gl),
                         seed=seed, shifts=24)
    if family == "coarse":
        return cf.search(grid_maker(st, 0.3), st.ts, w2("gradient", **gl) + w2("edge"), seed=seed)
    if family == "far":  # a 30 m long grid whose origin lies tens of metres from the robot (base shifted into it)
        return cf.search(grid_maker(st, 0.03, shape=(1024, 40, 40), anchor=(1, 0, 0)), st.ts, w2("gradient", **gl), seed=seed, shifts=24)
    if family == "switch":  # voxels only c_all / only c_obs holds, at the waypoints on either side of the standoff waypoint
        ts = st.ts
        return cf.search(grid_maker(st, 0.04), ts, [dict(kind="gradient", field="all", ts=[ts - 1], **gl),
                                                    dict(kind="gradient", field="obs", ts=[ts], **gl),
                                                    dict(kind="gradient", field="obs", ts=[ts - 1], **gl),   # the reverse:
                                                    dict(kind="gradient", field="all", ts=[ts], **gl)], seed=seed, shifts=24)
    raise ValueError(family)


ROBOT_ARGS = {"panda": dict(B=4, T=20, off=-4), "fetch": dict(B=4, T=20, off=-4, base=(0.0, 0.02, 0.01)),
              "wide9": dict(B=4, T=16, off=-3), "wide12": dict(B=4, T=16, off=-3), "wide16": dict(B=4, T=16, off=-3)}
FAMILIES = ["edge", "gradient", "near", "cap", "aniso1", "aniso2", "aniso3", "face", "coarse", "far", "switch"]


FAR_BASE = (29.0, -0.4, 0.3)  # the far family's base: the grid's origin lies about 30 m away along x
CAP_RES = 0.003


def contributing_fields(st, family, seed=0):
    """family_fields whose every design changes the oracle's obstacle terms at the seeds (a gradient across a point's only
    directions of motion contributes nothing: then the next seed's field).  Returns (fb, (Ao, go, sso))."""
    for s in range(seed, seed + 8):
        fb = family_fields(st, family, seed=s)
        st.o.set_scene(*fb.scene_args())
        ref = st.o.eval_obstacle_normal_eq(0, st.base, st.Q0)
        if all(contributes(fb, d, ref[0], ref[2]) for d in fb.designs):
            return fb, ref
    raise RuntimeError(f"no field of family {family} whose designs all contribute")


def obstacle_case(capi, om, robot, family, seed=0):
    kw = dict(ROBOT_ARGS[robot])
    if family == "far":
        kw["base"] = FAR_BASE
    if family == "cap":
        kw["cap_res"] = CAP_RES
    st = Setup(om, robot, seed=seed, **kw)
    fb, (Ao, go, sso) = contributing_fields(st, family, seed)
    h = st.handle(capi, om)
    h.set_scene(*fb.scene_args())
    h.set_profiling(True)
    A, g, ss = h.eval_obstacle_normal_eq(0, st.base, st.Q0)
    prof = h.last_kernel_profile()
    h.close()
    return dict(st=st, fb=fb, got=(A, g, ss), ref=(Ao, go, sso), prof=prof)


def contributes(fb, d, Ao, sso):
    """The oracle's obstacle terms at the design's waypoint are non-zero (a design in the other field: nothing required)."""
    if d.kind == "near" or d.field != fb.field_of(d.t):
        return True
    return bool(sso[d.b, d.t] > 0) if d.kind == "edge" else bool(np.abs(Ao[d.b, d.t]).max() > 0)


def obstacle_close(r):
    (A, g, ss), (Ao, go, sso) = r["got"], r["ref"]
    try:
        np.testing.assert_allclose(A[:, 2:], Ao[:, 2:], rtol=1e-8, atol=1e-10 * max(np.abs(Ao).max(), 1e-30))
        np.testing.assert_allclose(g[:, 2:], go[:, 2:], rtol=1e-8, atol=1e-10 * max(np.abs(go).max(), 1e-30))
        np.testing.assert_allclose(ss, sso, rtol=1e-11, atol=1e-15)
    except AssertionError as e:
        return str(e)
    return None


def cap_reached(st, fb):
    """The cap family reached its edges: chunks of R = 47, 48 and 49; the designed one's nearest record 30-47 voxels away;
    a chunk of R = 47 (culled: 48 > 47) and one of R >= 48 (never culled) facing the saturated distance 48."""
    geo = fb.geo
    assert [int(geo.R[l]) for l in st.cap_links] == [47, 48, 49]
    dist = {k: cf.chebyshev(cf.records_nonzero(a, geo.grid.shape)) for k, a in fb.fields.items()}
    d = fb.designs[0]
    assert d.R == 47 and 30 <= d.dist <= 47 and dist[d.field][d.centre] == d.dist
    seen = set()
    for b in range(geo.B):
        for t in range(2, geo.T):
            for l in st.cap_links:
                if dist[fb.field_of(t)][tuple(geo.kc[b, t, l])] == cf.CAP:
                    seen.add(min(int(geo.R[l]), 48))
    assert seen == {47, 48}, seen


OBSTACLE_CASES = ([(r, f) for r in ("panda", "fetch") for f in FAMILIES] +
                  [(r, f) for r in ("wide9", "wide12", "wide16") for f in ("edge", "gradient", "near", "aniso2", "switch")])


@pytest.mark.parametrize("robot,family", OBSTACLE_CASES)
def test_obstacle_normal_equations_on_culling_edges(capi, oracle_mod, record_property, robot, family):
    r = obstacle_case(capi, oracle_mod, robot, family)
    VARIANTS[f"obstacle {robot} {family}"] = _ran(r["prof"])
    record_property("kernel_variants", _ran(r["prof"]))
    if family == "cap":
        cap_reached(r["st"], r["fb"])
    if family == "face":  # the clipped-centre rule: every designed chunk's centre lies outside the grid
        assert all(r["fb"].geo.outside[d.b, d.t, d.link] for d in r["fb"].designs)
    (A, g, ss), (Ao, go, sso) = r["got"], r["ref"]
    if family == "near":  # every touched record is zero: exact zeros on both sides
        for x in (A, g, ss, Ao, go, sso):
            assert not np.any(x)
        return
    for d in r["fb"].designs:  # something to be found at every designed waypoint
        assert contributes(r["fb"], d, Ao, sso), d
    err = obstacle_close(r)
    assert err is None, err


# ------------------------------------------------------------------------------------------ the solve, step by step
SOLVE_CONFIGS = {
    # a few instances in flight: the few-instance obstacle variant and step kernel throughout
    "few": dict(B=6, env={}, families=("edge", "gradient")),
    # more than GTO_FEW_INSTANCES in flight: the step kernel's broad phase (prebroad_tail) settles waypoint groups
    "prebroad": dict(B=64, env={"GTO_FEW_INSTANCES": "16"}, families=("edge", "gradient")),
    # the same on a 30 m grid whose origin lies about 30 m from the base: large indices in prebroad_tail's float test,
    # against a widening (pb_eps) that follows the robot's size only
    "prebroad_far": dict(B=64, env={"GTO_FEW_INSTANCES": "16"}, families=("far",), base=FAR_BASE),
    # the same on anisotropic grids, one of them one voxel thin (strides of the separable distance field, clipped centres)
    "prebroad_aniso": dict(B=64, env={"GTO_FEW_INSTANCES": "16"}, families=("aniso1", "aniso2", "aniso3")),
    # the itemized obstacle launch laid out over 8 items: a crew of looping workgroups does nearly all of the work
    "sweep": dict(B=64, env={"GTO_FEW_INSTANCES": "16", "GTO_ITEM_HINT": "8"}, families=("edge", "gradient")),
    # voxels only one field holds, on either side of the standoff waypoint, with the step kernel's broad phase on
    "switch": dict(B=64, env={"GTO_FEW_INSTANCES": "16"}, families=("switch",)),
}


def solve_setup(om, config, robot="panda"):
    """The setup of a solve configuration and one field per family (each family gets its own scene and handle)."""
    c = SOLVE_CONFIGS[config]
    st = Setup(om, robot, B=c["B"], T=20, off=-4, seed=7, base=c.get("base", (0.0, 0.0, 0.0)))
    return st, [contributing_fields(st, f, seed=3)[0] for f in c["families"]]


def run_solve(capi, om, monkeypatch, config, max_iter, env=None):
    st, fbs = solve_setup(om, config)
    for k, v in (SOLVE_CONFIGS[config]["env"] if env is None else env).items():
        monkeypatch.setenv(k, v)
    out = []
    for fb in fbs:
        h = st.handle(capi, om, max_iter=max_iter)
        o = om.Oracle(st.desc, st.ee, st.gr, om.reference_opts(**dict(st.opts_kw, max_iter=max_iter)), n_gripper_points=st.ngp)
        for x in (h, o):
            x.set_scene(*fb.scene_args())
        h.set_profiling(True)
        got = h.solve_batch(*st.solve_args())
        prof = h.last_kernel_profile()
        ref = o.solve_batch(*st.solve_args())
        h.close()
        out.append(dict(got=got, ref=ref, prof=prof, fb=fb))
    return st, out


def solve_close(got, ref):
    Qg, _, fg, itg, stg = got
    Qo, _, fo, ito, sto = ref
    try:
        np.testing.assert_array_equal(itg, ito)
        np.testing.assert_array_equal(stg, sto)
        np.testing.assert_allclose(Qg, Qo, rtol=0, atol=1e-6)
        np.testing.assert_allclose(fg, fo, rtol=1e-8)
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize("config", list(SOLVE_CONFIGS))
@pytest.mark.parametrize("max_iter", [1, 2, 3, 25])
def test_solve_on_culling_edges_matches_oracle_every_instance(capi, oracle_mod, monkeypatch, record_property, config, max_iter):
    st, runs = run_solve(capi, oracle_mod, monkeypatch, config, max_iter)
    for fam, r in zip(SOLVE_CONFIGS[config]["families"], runs):
        VARIANTS[f"solve {config} {fam} max_iter={max_iter}"] = _ran(r["prof"])
        record_property(f"kernel_variants_{fam}", _ran(r["prof"]))
        if SOLVE_CONFIGS[config]["B"] > 16:
            assert r["prof"]["k_lm_step<4,1>"][1] > 0, r["prof"]  # the step kernel's broad phase ran
        else:
            assert r["prof"]["k_obstacle_gram<8,8>"][1] > 0 and r["prof"]["k_lm_step<4,1>"][1] == 0, r["prof"]
        err = solve_close(r["got"], r["ref"])
        assert err is None, (fam, err)
    if config == "sweep":
        # the crew ran: the itemized launches were laid out over 8 items instead of the estimate (fewer workgroups
        # launched), the same surface points were gathered, and the results are the bits of the launches without the hint
        monkeypatch.delenv("GTO_ITEM_HINT")
        _, plain = run_solve(capi, oracle_mod, monkeypatch, config, max_iter, env={"GTO_FEW_INSTANCES": "16"})
        for r, p in zip(runs, plain):
            for a, b in zip(r["got"], p["got"]):
                np.testing.assert_array_equal(a, b)
            k = "k_obstacle_gram<8,1>"
            assert r["prof"][k][3] == p["prof"][k][3] and r["prof"][k][2] < p["prof"][k][2], (r["prof"][k], p["prof"][k])


def test_designs_change_the_oracle_objective(oracle_mod):
    """The solve cases' fields are not empty where it matters: the oracle's obstacle terms at the designed waypoints."""
    for config in SOLVE_CONFIGS:
        st, fbs = solve_setup(oracle_mod, config)
        for fb in fbs:
            st.o.set_scene(*fb.scene_args())
            Ao, go, sso = st.o.eval_obstacle_normal_eq(0, st.base, st.Q0)
            assert all(contributes(fb, d, Ao, sso) for d in fb.designs), config


# ------------------------------------------------------------------------------------------ inverse kinematics
def ik_case(capi, om, family, robot="panda", seed=0):
    st = Setup(om, robot, B=6, T=20, off=-4, seed=11 + seed)
    q0 = st.qc + np.random.default_rng(5).uniform(-0.2, 0.2, st.qc.shape) * np.isin(np.arange(st.desc.ndof), st.desc.opt_index)
    Q = q0[:, :, None]  # one "waypoint": the seed the IK evaluates first
    gl = dict(links=st.moving, ts=[0])
    wants = {"edge": [dict(kind="edge", bs=[b], ts=[0]) for b in range(3)],
             "gradient": [dict(kind="gradient", bs=[b], **gl) for b in range(3)],
             # k_ik_solve reads the obstacle half only: voxels at the edge in c_all must change nothing
             "switch": [dict(kind="gradient", field="all", bs=[b], **gl) for b in range(3)] +
                       [dict(kind="gradient", field="obs", bs=[b], **gl) for b in range(3)]}[family]
    res = 0.1 if family == "edge" else 0.04
    lo, hi = st.box(np.repeat(Q, 2, axis=2))
    shape = tuple(int(x) for x in np.ceil((hi - lo + 0.3) / res))
    make = lambda shift: cf.Geometry(st.geo_o, st.desc, Q, st.base, cf.Grid(shape, tuple(lo - 0.15 + shift * res), res))
    fb = cf.search(make, 0, wants, seed=seed, shifts=24)  # ts = 0: every design of the default field is in c_obs
    h = st.handle(capi, om)
    for x in (h, st.o):
        x.set_scene(*fb.scene_args())
    got = h.solve_ik_batch(0, q0, st.goals[:, 0], st.base, max_iter=40)
    ref = st.o.solve_ik_batch(0, q0, st.goals[:, 0], st.base, max_iter=40)
    h.close()
    return dict(st=st, fb=fb, got=got, ref=ref, q0=q0)


def ik_close(got, ref):
    try:
        np.testing.assert_array_equal(got[2], ref[2])
        np.testing.assert_array_equal(got[3], ref[3])
        np.testing.assert_allclose(got[0], ref[0], rtol=0, atol=1e-6)
        np.testing.assert_allclose(got[1], ref[1], rtol=1e-8, atol=1e-12)
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize("family", ["edge", "gradient", "switch"])
def test_ik_on_culling_edges_matches_oracle(capi, oracle_mod, family):
    r = ik_case(capi, oracle_mod, family)
    err = ik_close(r["got"], r["ref"])
    assert err is None, err
    # something to be found: the oracle's IK with the field ends elsewhere than without it (obstacle half only)
    st = r["st"]
    free = st.o.solve_ik_batch(None, r["q0"], st.goals[:, 0], st.base, max_iter=40)
    moved = [b for b in range(st.B) if not np.array_equal(free[0][b], r["ref"][0][b])]
    if family == "switch":
        assert moved, "the c_obs designs change nothing"
    else:
        assert set(d.b for d in r["fb"].designs) <= set(moved), moved


# ------------------------------------------------------------------------------------------ distance-field constructions
@pytest.mark.parametrize("family", ["aniso1", "aniso2", "aniso3", "face", "far"])
def test_relaxed_and_separable_distance_fields_cull_alike_on_sparse_grids(capi, oracle_mod, monkeypatch, family):
    """GTO_DIST_RELAX=1 builds the field by GTO_DIST_CAP sweeps of min-plus-one, the default by one pass per axis: on
    anisotropic, one-voxel-thin and far-away grids they cull the same chunks (equal work) and give the same bits."""
    kw = dict(ROBOT_ARGS["panda"], B=24)
    if family == "far":
        kw["base"] = FAR_BASE
    st = Setup(oracle_mod, "panda", **kw)
    fb = family_fields(st, family)
    res = []
    for env in ({}, {"GTO_DIST_RELAX": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        h = st.handle(capi, oracle_mod, max_iter=15)
        h.set_scene(*fb.scene_args())
        h.set_profiling(True)
        out = h.solve_batch(*st.solve_args())
        res.append((out, h.last_kernel_work()[0]))
        h.close()
    for a, b in zip(res[0][0], res[1][0]):
        np.testing.assert_array_equal(a, b)
    assert res[0][1] == res[1][1] and res[0][1] > 0


# ------------------------------------------------------------------------------------------ shared halves
def test_shared_halves_follow_their_fields(capi, oracle_mod):
    """gto_share_scene_halves: the destination's c_all / c_obs are the source's field all_from / obs_from, and so are
    the records and distance fields its broad phases cull by.  The source's two fields differ exactly at designed edges:
    a gradient design in each field at a waypoint before the standoff waypoint and one after it, for the solve, and one in
    each field at the IK's seed (instances B and B + 1 of the geometry: the seed held over the horizon), for the IK."""
    st = Setup(oracle_mod, "panda", B=6, T=20, off=-4, seed=21)
    ts, gl, B = st.ts, dict(links=st.moving), st.B
    q0 = st.qc.copy()
    Qx = np.concatenate([st.Q0, np.repeat(q0[:2, :, None], st.T, axis=2)])
    bx = np.concatenate([st.base, st.base[:2]])
    lo, hi = st.box()  # (the seeds start next to qc)
    shape, org = tuple(int(x) for x in np.ceil((hi - lo + 0.3) / 0.04)), lo - 0.15
    make = lambda shift: cf.Geometry(st.geo_o, st.desc, Qx, bx, cf.Grid(shape, tuple(org + shift * 0.04), 0.04))
    wants = [dict(kind="gradient", field=f, bs=list(range(B)), ts=t, **gl)
             for f in ("all", "obs") for t in (list(range(2, ts)), list(range(ts, st.T)))] * 2
    wants += [dict(kind="gradient", field=f, bs=[B + i], ts=[2], **gl) for i, f in enumerate(("all", "obs"))]
    fb = cf.search(make, ts, wants, seed=4, shifts=24)
    ik_designs = [d for d in fb.designs if d.b >= B]
    _, ca, co, shape, origin, res = fb.scene_args()
    assert np.any(ca != co)
    src = st.handle(capi, oracle_mod, max_iter=12)
    src.set_scene(0, ca, co, shape, origin, res)
    fa, fo = src.scene_fields(0)
    np.testing.assert_array_equal(fa, ca)
    np.testing.assert_array_equal(fo, co)
    free = oracle_mod.Oracle(st.desc, st.ee, st.gr, oracle_mod.reference_opts(**st.opts_kw)).solve_ik_batch(
        None, q0, st.goals[:, 0], st.base, max_iter=30)
    for all_from in (0, 1):
        for obs_from in (0, 1):
            pick = (ca, co)
            dst = st.handle(capi, oracle_mod, max_iter=12)
            dst.share_scene(0, src, 0, all_from=all_from, obs_from=obs_from)
            da, do = dst.scene_fields(0)
            np.testing.assert_array_equal(da, pick[all_from])
            np.testing.assert_array_equal(do, pick[obs_from])
            o = oracle_mod.Oracle(st.desc, st.ee, st.gr, oracle_mod.reference_opts(**dict(st.opts_kw, max_iter=12)))
            o.set_scene(0, pick[all_from], pick[obs_from], shape, origin, res)
            err = solve_close(dst.solve_batch(*st.solve_args()), o.solve_batch(*st.solve_args()))
            assert err is None, ((all_from, obs_from), err)
            ref = o.solve_ik_batch(0, q0, st.goals[:, 0], st.base, max_iter=30)
            err = ik_close(dst.solve_ik_batch(0, q0, st.goals[:, 0], st.base, max_iter=30), ref)
            assert err is None, ((all_from, obs_from), err)
            # something to be found: the IK design in the half the IK reads moves its instance's oracle result
            for d in ik_designs:
                if d.field == ("all", "obs")[obs_from]:
                    assert not np.array_equal(ref[0][d.b - B], free[0][d.b - B]), ((all_from, obs_from), d)
            dst.close()
    # a set_scene that replaces the source: the source returns the new arrays; a destination shared again follows them
    ca2, co2 = co.copy(), ca.copy()
    src.set_scene(0, ca2, co2, shape, origin, res)
    fa, fo = src.scene_fields(0)
    np.testing.assert_array_equal(fa, ca2)
    np.testing.assert_array_equal(fo, co2)
    dst = st.handle(capi, oracle_mod, max_iter=12)
    dst.share_scene(0, src, 0, all_from=1, obs_from=0)
    da, do = dst.scene_fields(0)
    np.testing.assert_array_equal(da, co2)
    np.testing.assert_array_equal(do, ca2)
    o = oracle_mod.Oracle(st.desc, st.ee, st.gr, oracle_mod.reference_opts(**dict(st.opts_kw, max_iter=12)))
    o.set_scene(0, co2, ca2, shape, origin, res)
    err = solve_close(dst.solve_batch(*st.solve_args()), o.solve_batch(*st.solve_args()))
    assert err is None, err
    dst.close()
    src.close()


# ------------------------------------------------------------------------------------------ the margin -1 mutant
def mutant_report(out_path):
    """Run the edge-field cases of each consumer family with the library in use; write which assertions fail.  (The margin
    applies to every broad phase at once: what catches it in the prebroad solve may be the obstacle kernel's test of the
    seeds, which k_obstacle_gram evaluates, and not prebroad_tail's own test of the trial trajectories.)"""
    import __graft_entry__  # noqa: F401  (puts the repository on sys.path)
    from grasptrajopt_amd import _capi
    from oracle import oracle as om

    class MP:  # monkeypatch stand-in: this runs in its own process
        def setenv(self, k, v):
            os.environ[k] = v

    rep = {}
    for robot in ("panda", "wide12"):
        for fam in ("edge", "gradient"):
            rep[f"obstacle {robot} {fam}"] = obstacle_close(obstacle_case(_capi, om, robot, fam))
    st, runs = run_solve(_capi, om, MP(), "prebroad", 25)
    rep["solve prebroad"] = " | ".join(filter(None, (solve_close(r["got"], r["ref"]) for r in runs))) or None
    rep["solve prebroad ran k_lm_step<4,1>"] = all(r["prof"]["k_lm_step<4,1>"][1] > 0 for r in runs)
    for fam in ("edge", "gradient"):
        r = ik_case(_capi, om, fam)
        rep[f"ik {fam}"] = ik_close(r["got"], r["ref"])
    with open(out_path, "w") as fh:
        json.dump(rep, fh)


@pytest.fixture(scope="module")
def margin_mutant(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("mut") / "libgto_hip_margin.so")
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    src = [os.path.join(g.CSRC, s) for s in g.HIP_SOURCES]
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + g.HIPCC_FLAGS + ["-DGTO_BROAD_MARGIN=-1"] + src + ["-o", lib],
                       cwd=g.CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return lib


def test_margin_minus_one_is_caught_by_every_consumer_family(capi, margin_mutant, tmp_path):
    out = str(tmp_path / "mutant.json")
    env = dict(os.environ, GTO_HIP_LIB=margin_mutant)
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
            f"import test_gpu_culling as t; t.mutant_report({out!r})")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rep = json.load(open(out))
    print("\nmargin -1 mutant, what caught it:\n" + "\n".join(f"  {k}: {str(v)[:160]!r}" for k, v in rep.items()))
    assert rep["solve prebroad ran k_lm_step<4,1>"]
    for k, v in rep.items():
        if not k.endswith("k_lm_step<4,1>"):
            assert v, f"{k}: the margin -1 library agrees with the oracle"
