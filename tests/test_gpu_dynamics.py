"""gto_set_link_inertials and gto_inverse_dynamics (csrc/gto_dynamics.h, k_inverse_dynamics) against tests/dynamics_ref.py,
which tests/test_dynamics_cpu.py holds against physics.

Robots: Panda and Fetch (the fixtures' inertials; Fetch has a prismatic torso and fingers and lumped pruned links), a
branched tree with a fixed frame inside a branch, a chain with prismatic joints, and the edge robots of
tests/dynamics_cases.py (seeded bodies): one frame whose root is actuated and carries the payload, two, three (no revolute
joint) and four frames (the payload on the fixed root, above every joint), ten frames, and two robots of 32 frames (a chain
of 31 joints, a bushy tree).  A workgroup holds rows_per_block(F) = min(64, 65536 // (15 * F * 8)) rows of a robot of F
frames (csrc/gto_dynamics.h: GTO_RNEA_LDS_BYTES / (GTO_RNEA_SLOTS * F * sizeof(double)), at most a wave): 64 up to eight
frames, 45 on Panda's twelve, 17 at 32.  n = 67 rows is more than one workgroup on every one of them and a multiple of none
of these counts (four workgroups with a ragged last one at 32 frames); n = 1 is the other end.  The rows: seeded in-limit states, then rows at the lower and the upper limits, rows at rest
(qd = 0), and static rows (qd = qdd = 0).  Agreement: 1e-11 relative to max(1, |tau|_inf), the project's FP64 parity bar.
"""
import ctypes as C

import numpy as np
import pytest

import dynamics_cases as dc
import dynamics_ref as dr

pytestmark = pytest.mark.gpu

N = 67


def rows_per_block(F):
    """rnea_rows_per_block of csrc/gto_dynamics.h, restated from its constants."""
    return min(64, (64 * 1024) // (15 * F * 8))


def single_rows(F):
    """The first row, the row that starts the second workgroup of a robot of F frames, the last."""
    rows = rows_per_block(F)
    return (0, rows if rows < N else 33, N - 1)


def test_the_robots_cover_the_layouts():
    F = {name: dc.robot(name)[0].n_frames for name in dc.NAMES}
    rows = {rows_per_block(f) for f in F.values()}
    assert 1 in F.values() and 64 in rows and 17 in rows and max(F.values()) == 32
    assert all(0 < r < N and N % r != 0 for r in rows)  # more than one workgroup, the last one ragged, on every robot


@pytest.fixture(scope="module")
def capi():
    from grasptrajopt_amd import _capi
    return _capi


def states(desc):
    q, qd, qdd = dr.in_limit_states(desc, N, seed=21)
    lo, hi = q.min(axis=0), q.max(axis=0)
    opt = np.asarray(desc.opt_index)
    lo[opt], hi[opt] = np.maximum(desc.lower[opt], -2 * np.pi), np.minimum(desc.upper[opt], 2 * np.pi)
    q[60], q[61] = lo, hi          # at the limits
    qd[62:65] = 0.0                # at rest
    qd[65:] = qdd[65:] = 0.0       # static: tau = g
    return q, qd, qdd


@pytest.fixture(scope="module", params=dc.NAMES)
def case(request, capi):
    desc, ee, gr, ngp = dc.robot(request.param)
    h = capi.SolverHandle(desc, ee, gr, device=0, n_gripper_points=ngp)
    q, qd, qdd = states(desc)
    pls = dc.payloads(N, seed=22)
    ref = {k: dr.inverse_dynamics_rows(desc, q, qd, qdd, desc.frame_index(ee), pl) for k, pl in pls.items()}  # computed once
    yield dict(name=request.param, desc=desc, h=h, q=q, qd=qd, qdd=qdd, payloads=pls, ref=ref)
    h.close()


def as_dict(pl, rows=slice(None)):
    if pl is None:
        return None
    return {k: v[rows] for k, v in zip(("mass", "com", "inertia"), pl) if v is not None}


@pytest.mark.parametrize("kind", ["none", "mass", "full"])
def test_inverse_dynamics_matches_the_reference(case, kind):
    pl = case["payloads"][kind]
    tau = case["h"].inverse_dynamics(case["q"], case["qd"], case["qdd"], as_dict(pl))
    ref = case["ref"][kind]
    assert tau.shape == ref.shape and np.isfinite(tau).all()
    err = np.abs(tau - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))
    print(f"{case['name']} {kind}: max relative error {err.max():.3e}, |tau|_inf {np.abs(ref).max():.3f}")
    assert err.max() <= 1e-11
    if kind != "none":  # the payload is felt (but for the row whose payload mass is 0, and where no joint can feel it)
        base = case["ref"]["none"]
        assert np.array_equal(tau[2], case["h"].inverse_dynamics(case["q"][2], case["qd"][2], case["qdd"][2])[0])
        if (case["name"], kind) in dc.PAYLOAD_NOT_FELT:
            assert np.abs(ref - base).max() <= 1e-12
        else:
            assert np.abs(ref - base).max() > 1e-3
    for i in single_rows(case["desc"].n_frames):  # a row alone is the row inside the batch, bit for bit
        one = case["h"].inverse_dynamics(case["q"][i], case["qd"][i], case["qdd"][i], as_dict(pl, slice(i, i + 1)))
        assert np.array_equal(one[0], tau[i]), (kind, i)


def test_gravity_and_repeated_upload(case):
    d, h = case["desc"], case["h"]
    q, z = case["q"][:5], np.zeros((5, d.ndof))
    try:
        h.set_link_inertials(d.frame_mass, d.frame_com, d.frame_inertia, gravity=[0, 0, 0])
        assert np.abs(h.inverse_dynamics(q, z, z)).max() == 0.0  # nothing to hold without gravity
        g = np.array([1.5, -2.0, -7.0])
        h.set_link_inertials(d.frame_mass, d.frame_com, d.frame_inertia, gravity=g)
        ref = np.stack([dr.inverse_dynamics(d, q[i], case["qd"][i], case["qdd"][i], gravity=g) for i in range(5)])
        tau = h.inverse_dynamics(q, case["qd"][:5], case["qdd"][:5])
        assert (np.abs(tau - ref).max(axis=1) <= 1e-11 * np.maximum(1.0, np.abs(ref).max(axis=1))).all()
    finally:
        h.set_link_inertials(d.frame_mass, d.frame_com, d.frame_inertia)
    assert np.array_equal(h.inverse_dynamics(q, z, z), h.inverse_dynamics(case["q"], 0 * case["q"], 0 * case["q"])[:5])


def test_errors_leave_the_handle_and_the_outputs_alone(capi):
    from grasptrajopt_amd.robot_desc import load_builtin
    desc, ee, gr, _ = dc.robot("panda")
    plain = load_builtin("panda")
    h = capi.SolverHandle(plain, ee, gr, device=0)
    q = np.zeros((2, desc.ndof))
    with pytest.raises(capi.GTOError, match=r"\(-1\): no link inertials set$"):
        h.inverse_dynamics(q, q, q)
    h.set_link_inertials(desc.frame_mass, desc.frame_com, desc.frame_inertia)
    good = h.inverse_dynamics(q, q, q)
    F = desc.n_frames
    bad_mass, bad_nan, bad_inertia, bad_com = desc.frame_mass.copy(), desc.frame_mass.copy(), desc.frame_inertia.copy(), desc.frame_com.copy()
    bad_mass[3], bad_nan[4], bad_com[2, 1] = -1.0, np.nan, np.inf
    bad_inertia[5] = [0.01, 0.0, 0.0, -0.02, 0.0, 0.01]  # a negative principal moment
    for args, why in (((bad_mass, desc.frame_com, desc.frame_inertia), "link mass must be >= 0 and finite"),
                      ((bad_nan, desc.frame_com, desc.frame_inertia), "link mass must be >= 0 and finite"),
                      ((desc.frame_mass, bad_com, desc.frame_inertia), "non-finite centre of mass"),
                      ((desc.frame_mass, desc.frame_com, bad_inertia), "link inertia must be symmetric positive semidefinite")):
        with pytest.raises(capi.GTOError, match=rf"\(-1\): {why}$"):
            h.set_link_inertials(*args)
    with pytest.raises(capi.GTOError, match=r"\(-1\): non-finite gravity$"):
        h.set_link_inertials(desc.frame_mass, desc.frame_com, desc.frame_inertia, gravity=[0, np.nan, 0])
    massless = desc.frame_mass.copy()  # a massless frame's other entries are ignored, garbage included
    massless[F - 1] = 0.0
    junk_com, junk_inertia = desc.frame_com.copy(), desc.frame_inertia.copy()
    junk_com[F - 1], junk_inertia[F - 1] = np.nan, -1.0
    h.set_link_inertials(massless, junk_com, junk_inertia)
    assert np.isfinite(h.inverse_dynamics(q, q, q)).all()
    h.set_link_inertials(desc.frame_mass, desc.frame_com, desc.frame_inertia)
    assert np.array_equal(h.inverse_dynamics(q, q, q), good)  # the refused calls changed nothing
    # the C ABI's own refusals (the Python layer checks a payload before it calls): outputs untouched
    pd = C.POINTER(C.c_double)
    out = np.full((2, desc.ndof), 7.0)
    neg = np.array([1.0, -0.5])
    p = lambda a: None if a is None else a.ctypes.data_as(pd)  # noqa: E731
    for mass, com, why in ((neg, None, "payload mass must be >= 0 and finite"),
                           (np.array([np.nan, 1.0]), None, "payload mass must be >= 0 and finite"),
                           (None, np.zeros((2, 3)), "payload_com / payload_inertia without payload_mass")):
        rc = h.lib.gto_inverse_dynamics(h._h, 2, p(q), p(q), p(q), p(mass), p(com), None, p(out))
        assert rc == -1 and h.lib.gto_last_error(h._h).decode() == why
        assert (out == 7.0).all()
    assert h.lib.gto_inverse_dynamics(h._h, 0, None, None, None, None, None, None, None) == 0
    assert h.lib.gto_inverse_dynamics(h._h, -1, p(q), p(q), p(q), None, None, None, p(out)) == -1
    h.close()


@pytest.mark.parametrize("name", ["panda", "fetch"])
def test_python_layers_call_the_same_entry_point(name, capi):
    from grasptrajopt_amd import utils
    from grasptrajopt_amd.gto_models import GTORobotModel
    from grasptrajopt_amd.robot_desc import load_builtin
    d, ee, gr, _ = dc.robot(name)
    h = capi.SolverHandle(d, ee, gr, device=0)
    q, qd, qdd = dr.in_limit_states(d, 9, seed=23)
    robot = GTORobotModel(desc=d, device=0)
    pl = as_dict(dc.payloads(9, seed=24)["full"])
    tau = utils.inverse_dynamics(robot, q, qd, qdd, payload=pl, link_ee=ee)
    assert np.array_equal(tau, h.inverse_dynamics(q, qd, qdd, pl))
    one = utils.inverse_dynamics(robot, q[3], qd[3], qdd[3])
    assert one.shape == (d.ndof,) and np.array_equal(one, h.inverse_dynamics(q[3], qd[3], qdd[3])[0])
    with pytest.raises(ValueError, match="needs link_ee"):
        utils.inverse_dynamics(robot, q[3], qd[3], qdd[3], payload={"mass": 1.0})
    bare = GTORobotModel(desc=load_builtin(name), device=0)  # a packaged description: no inertials until they are set
    with pytest.raises(ValueError, match="no link inertials"):
        utils.inverse_dynamics(bare, q, qd, qdd)
    eff = np.asarray(robot.effort_optimized_joint_limits.toarray()).ravel()
    assert np.array_equal(eff, d.effort[d.opt_index])
    h.close()
    for hh in robot._handles.values():
        hh.close()
