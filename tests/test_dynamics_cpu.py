"""tests/dynamics_ref.py, the yardstick of gto_inverse_dynamics, held against physics rather than against itself; the URDF
reader's inertial and effort fields; the lumping of pruned links (no GPU here).

Three checks per robot (Panda and Fetch with the fixtures' inertials; a branched tree, a chain with prismatic joints and the
edge robots of tests/dynamics_cases.py with seeded bodies: one frame with an actuated root, no revolute joint, a payload on
a frame above the joints, 32 frames with 31 joints) over 32 seeded in-limit states (the first 8 of them on the two robots of
32 frames, FEWER_STATES), half of them with a payload on the end effector:
  1. ID(q, 0, e_j) - g, stacked, is the mass matrix sum_k m_k Jv_k^T Jv_k + Jw_k^T R_k I_k R_k^T Jw_k, built here from the
     frames' world axes (the geometric Jacobian of every body's centre of mass) and not from the recursion: 1e-12 relative.
     It is symmetric, and positive definite on the joints that move mass.
  2. g is the gradient of the potential energy V = -sum_k m_k g . c_k, by central differences.
  3. tau . qd is d/dt (T + V) along a seeded smooth q(t), T = qd^T M qd / 2 with the M of check 1, by central differences.

Tolerances of 2 and 3.  A central difference D(h) of step h errs by h^2 f''' / 6 + O(h^4), so D(h) - D(h/2) is 3/4 of D(h)'s
error and 3 times that of D(h/2).  The tests compare against D(h/2) and allow TRUNC_SAFETY = 4 times its estimated error
|D(h) - D(h/2)| / 3 (the largest over the components: one component's estimate may vanish by chance), plus the round-off of
the difference quotient, ROUND_ULPS = 16 units of 2^-52 max|f| / (h/2).  Both constants were chosen before the first run.
The forward kinematics under all three is compared with the oracle's first.
"""
import numpy as np
import pytest

import dynamics_cases as dc
import dynamics_ref as dr

N_STATES = 32
# the two robots of 32 frames take a third of a second per state in the finite-difference checks: the first 8 states there
FEWER_STATES = {"limit_chain": 8, "limit_bushy": 8}
H = 1e-3
TRUNC_SAFETY, ROUND_ULPS = 4.0, 16.0
EPS = 2.0 ** -52


@pytest.fixture(scope="module", params=dc.NAMES)
def case(request):
    desc, ee, gr, ngp = dc.robot(request.param)
    q, qd, qdd = dr.in_limit_states(desc, N_STATES, seed=5)
    pl = dc.payloads(N_STATES, seed=6)["full"]
    payload = [None if i % 2 == 0 else (pl[0][i], pl[1][i], pl[2][i]) for i in range(N_STATES)]
    return dict(name=request.param, desc=desc, ee=desc.frame_index(ee), link_ee=ee, link_gripper=gr, ngp=ngp, q=q, qd=qd, qdd=qdd,
                payload=payload, n=FEWER_STATES.get(request.param, N_STATES))


def mass_matrix(desc, q, ee, payload):
    """sum over the bodies of m Jv^T Jv + Jw^T R I R^T Jw, columns from the world axes of the joints above each body."""
    R, p, z = dr.fk(desc, q)
    M = np.zeros((desc.ndof, desc.ndof))
    for f, m, c, I in dr.bodies(desc, ee, payload):
        pc = p[f] + R[f] @ c
        Jv, Jw = np.zeros((3, desc.ndof)), np.zeros((3, desc.ndof))
        g = f
        while g >= 0:
            if desc.joint_type[g] == dr.REVOLUTE:
                Jv[:, desc.q_index[g]] = np.cross(z[g], pc - p[g])
                Jw[:, desc.q_index[g]] = z[g]
            elif desc.joint_type[g] == dr.PRISMATIC:
                Jv[:, desc.q_index[g]] = z[g]
            g = desc.parent[g]
        M += m * Jv.T @ Jv + Jw.T @ R[f] @ I @ R[f].T @ Jw
    return M


def potential(desc, q, ee, payload):
    R, p, _ = dr.fk(desc, q)
    return -sum(m * dr.GRAVITY @ (p[f] + R[f] @ c) for f, m, c, I in dr.bodies(desc, ee, payload))


def central(f, x, h):
    """Central differences of f along every coordinate of x (or along the scalar x)."""
    if np.ndim(x) == 0:
        return (f(x + h) - f(x - h)) / (2 * h)
    out = np.zeros(len(x))
    for j in range(len(x)):
        e = np.zeros(len(x))
        e[j] = h
        out[j] = (f(x + e) - f(x - e)) / (2 * h)
    return out


def difference_tolerance(d_h, d_h2, fmax):
    return TRUNC_SAFETY * np.max(np.abs(d_h - d_h2)) / 3.0 + ROUND_ULPS * EPS * fmax / (H / 2)


def test_forward_kinematics_of_the_yardstick(case, oracle_mod):
    d = case["desc"]
    orc = oracle_mod.Oracle(d, case["link_ee"], case["link_gripper"], oracle_mod.reference_opts(), n_gripper_points=case["ngp"])
    X = orc.eval_fk(case["q"])
    for i in range(case["n"]):
        R, p, _ = dr.fk(d, case["q"][i])
        np.testing.assert_allclose(R, X[i, :, :3, :3], rtol=0, atol=1e-12)
        np.testing.assert_allclose(p, X[i, :, :3, 3], rtol=0, atol=1e-12)


def test_unit_accelerations_give_the_mass_matrix(case):
    d, ee = case["desc"], case["ee"]
    zero = np.zeros(d.ndof)
    for i in range(case["n"]):
        q, pl = case["q"][i], case["payload"][i]
        g = dr.inverse_dynamics(d, q, zero, zero, ee, pl)
        M = np.stack([dr.inverse_dynamics(d, q, zero, e, ee, pl) - g for e in np.eye(d.ndof)], axis=1)
        Mref = mass_matrix(d, q, ee, pl)
        scale = np.abs(Mref).max()
        assert np.abs(M - Mref).max() <= 1e-12 * scale, (case["name"], i)
        assert np.abs(Mref - Mref.T).max() <= 1e-14 * scale
        moving = np.diag(Mref) > 0
        assert moving.sum() >= min(d.ndof, 2)
        assert np.linalg.eigvalsh(Mref[np.ix_(moving, moving)]).min() > 0


def test_static_torques_are_the_gradient_of_the_potential(case):
    d, ee = case["desc"], case["ee"]
    zero = np.zeros(d.ndof)
    for i in range(case["n"]):
        q, pl = case["q"][i], case["payload"][i]
        g = dr.inverse_dynamics(d, q, zero, zero, ee, pl)
        V = lambda x: potential(d, x, ee, pl)  # noqa: E731
        d_h, d_h2 = central(V, q, H), central(V, q, H / 2)
        tol = difference_tolerance(d_h, d_h2, abs(V(q)))
        assert np.abs(g - d_h2).max() <= tol, (case["name"], i, np.abs(g - d_h2).max(), tol)
        assert tol < 1e-4 * max(1.0, np.abs(g).max())  # the comparison is a sharp one


def test_power_is_the_rate_of_the_energy(case):
    d, ee = case["desc"], case["ee"]
    rng = np.random.default_rng(9)
    for i in range(case["n"]):
        pl = case["payload"][i]
        q0, amp = case["q"][i], rng.uniform(0.05, 0.3, d.ndof)
        om, ph = rng.uniform(0.5, 2.0, d.ndof), rng.uniform(0, 2 * np.pi, d.ndof)
        qt = lambda t: q0 + amp * (np.sin(om * t + ph) - np.sin(ph))  # noqa: E731
        qdt = lambda t: amp * om * np.cos(om * t + ph)  # noqa: E731
        qddt = lambda t: -amp * om * om * np.sin(om * t + ph)  # noqa: E731

        def energy(t):
            v = qdt(t)
            return 0.5 * v @ mass_matrix(d, qt(t), ee, pl) @ v + potential(d, qt(t), ee, pl)

        t0 = 0.37
        tau = dr.inverse_dynamics(d, qt(t0), qdt(t0), qddt(t0), ee, pl)
        d_h, d_h2 = central(energy, t0, H), central(energy, t0, H / 2)
        tol = difference_tolerance(np.array([d_h]), np.array([d_h2]), abs(energy(t0)))
        assert abs(tau @ qdt(t0) - d_h2) <= tol, (case["name"], i, abs(tau @ qdt(t0) - d_h2), tol)
        assert tol < 1e-4 * max(1.0, abs(d_h2))


# ------------------------------------------------------------------------------------------------ URDF reader, lumping
URDF = """<robot name="r">
 <link name="base"><inertial><origin xyz="0 0 0.1"/><mass value="5"/><inertia ixx="1" iyy="1" izz="1"/></inertial></link>
 <link name="l1"><inertial><origin xyz="0.1 0.02 0.03" rpy="0.3 -0.2 0.5"/><mass value="2"/>
   <inertia ixx="0.02" ixy="0.001" ixz="-0.002" iyy="0.03" iyz="0.0015" izz="0.01"/></inertial></link>
 <link name="l2"><inertial><mass value="1.5"/><inertia ixx="0.01" ixy="0" ixz="0" iyy="0.01" iyz="0" izz="0.02"/></inertial></link>
 <link name="tool"><inertial><origin xyz="0 0.05 0.1" rpy="0 0.4 0"/><mass value="0.7"/>
   <inertia ixx="0.004" ixy="0.0005" ixz="0" iyy="0.003" iyz="0" izz="0.002"/></inertial></link>
 <link name="side"><inertial><origin xyz="0.03 0 0"/><mass value="0.4"/><inertia ixx="0.001" iyy="0.002" izz="0.003"/></inertial></link>
 <link name="tip"/>
 <joint name="j1" type="revolute"><parent link="base"/><child link="l1"/><origin xyz="0 0 0.2" rpy="0.1 0.2 0"/><axis xyz="0 1 0"/>
   <limit lower="-1" upper="1" velocity="2" effort="40"/></joint>
 <joint name="j2" type="revolute"><parent link="l1"/><child link="l2"/><origin xyz="0.3 0 0" rpy="0 0 0.4"/><axis xyz="1 0 0"/>
   <limit lower="-1" upper="1" velocity="2"/></joint>
 <joint name="jt" type="fixed"><parent link="l2"/><child link="tool"/><origin xyz="0.1 0 0.05" rpy="0.2 0 -0.3"/></joint>
 <joint name="j3" type="prismatic"><parent link="l1"/><child link="side"/><origin xyz="0 0.1 0" rpy="0 0.5 0"/><axis xyz="0 0 1"/>
   <limit lower="-0.1" upper="0.1" velocity="1" effort="15"/></joint>
 <joint name="j4" type="continuous"><parent link="tool"/><child link="tip"/></joint>
</robot>"""


def test_urdf_inertial_and_effort_fields():
    from grasptrajopt_amd.robot_desc import RobotDesc, link_inertial_in_link_frame, _rpy_matrix, _sym3
    from grasptrajopt_amd.urdf import Urdf
    u = Urdf.from_string(URDF)
    l1 = u.link_map["l1"]
    assert l1.mass == 2.0 and l1.inertial_xyz == [0.1, 0.02, 0.03] and l1.inertial_rpy == [0.3, -0.2, 0.5]
    assert l1.inertia == [0.02, 0.001, -0.002, 0.03, 0.0015, 0.01]
    assert u.link_map["base"].inertia == [1, 0, 0, 1, 0, 1] and u.link_map["base"].inertial_rpy == [0, 0, 0]
    assert u.link_map["tip"].mass == 0.0
    assert [u.joint_map[j].effort for j in ("j1", "j2", "j3", "j4")] == [40.0, 0.0, 15.0, 1e9]
    # the inertial origin's rpy turns the tensor into the link frame: the same kinetic energy for a spin stated in either
    m, c, I = link_inertial_in_link_frame(l1)
    R = _rpy_matrix(l1.inertial_rpy)
    w_link = np.array([0.3, -1.1, 0.7])
    assert abs(w_link @ I @ w_link - (R.T @ w_link) @ _sym3(l1.inertia) @ (R.T @ w_link)) < 1e-15
    assert np.abs(I - I.T).max() <= 4 * EPS * np.abs(I).max()  # R I R^T in floating point: symmetric to round-off
    d = RobotDesc.from_urdf(u, keep_all_frames=True)
    assert d.actuated_joint_names == ["j1", "j2", "j3", "j4"]
    np.testing.assert_array_equal(d.effort, [40.0, np.inf, 15.0, np.inf])
    f = d.frame_index("l1")
    assert d.frame_mass[f] == 2.0
    np.testing.assert_array_equal(d.frame_com[f], [0.1, 0.02, 0.03])
    np.testing.assert_allclose(_sym3(d.frame_inertia[f]), I, rtol=0, atol=1e-17)
    assert d.frame_mass[d.frame_index("tip")] == 0.0
    from grasptrajopt_amd.gto_models import GTORobotModel  # the limits beside the velocity limits
    assert hasattr(GTORobotModel, "effort_optimized_joint_limits") and hasattr(GTORobotModel, "effort_actuated_joint_limits")


def test_pruned_links_are_lumped_into_their_kept_ancestor():
    """Total mass, and the static torques with the pruned joints at 0, are those of the description that keeps every frame."""
    from grasptrajopt_amd.robot_desc import RobotDesc
    from grasptrajopt_amd.urdf import Urdf
    u = Urdf.from_string(URDF)
    full = RobotDesc.from_urdf(u, keep_all_frames=True)
    cut = RobotDesc.from_urdf(u, extra_links=["l2"])
    assert cut.frame_names == ["base", "l1", "l2"] and full.n_frames == 6
    # (five additions in another order: a few units of 2^-52 * 9.6 = 2e-15)
    assert abs(cut.frame_mass.sum() - full.frame_mass.sum()) < 1e-14 and abs(full.frame_mass.sum() - 9.6) < 1e-14
    assert cut.frame_mass[1] == pytest.approx(2.4, abs=1e-15) and cut.frame_mass[2] == pytest.approx(2.2, abs=1e-15)
    rng = np.random.default_rng(3)
    zero = np.zeros(4)
    for _ in range(8):
        q = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), 0.0, 0.0])  # j3 and j4 are pruned: taken at 0
        np.testing.assert_allclose(dr.inverse_dynamics(cut, q, zero, zero)[:2], dr.inverse_dynamics(full, q, zero, zero)[:2],
                                   rtol=0, atol=1e-13)
        # rigidly welded, the lumped body also has the pruned subtree's inertia: the same forces when j1 and j2 accelerate
        qd, qdd = np.array([0.7, -0.4, 0, 0]), np.array([1.3, 0.9, 0, 0])
        np.testing.assert_allclose(dr.inverse_dynamics(cut, q, qd, qdd)[:2], dr.inverse_dynamics(full, q, qd, qdd)[:2],
                                   rtol=0, atol=1e-13)


def test_descriptions_carry_inertials_when_present(tmp_path):
    from grasptrajopt_amd.robot_desc import RobotDesc, load_builtin, with_planar_base
    d = load_builtin("panda")
    assert not d.has_inertials and d.effort is None  # the packaged descriptions are as they were
    d.save(str(tmp_path / "plain"))
    assert not RobotDesc.load(str(tmp_path / "plain")).has_inertials
    d = dr.with_fixture_inertials(d, "panda")
    assert d.frame_mass[d.frame_index("panda_link5")] == 3.5 and d.effort[1] == 87.0 and d.effort[4] == 12.0
    d.save(str(tmp_path / "dyn"))
    e = RobotDesc.load(str(tmp_path / "dyn"))
    for k in ("frame_mass", "frame_com", "frame_inertia", "effort"):
        np.testing.assert_array_equal(getattr(e, k), getattr(d, k))
    m = with_planar_base(d)
    assert m.frame_mass.shape == (d.n_frames + 4,) and m.frame_mass[:4].sum() == 0 and np.isinf(m.effort[:3]).all()
    with pytest.raises(ValueError):
        d.set_link_inertials(np.zeros(3), np.zeros((3, 3)), np.zeros((3, 6)))


def test_fetch_fixture_lumps_the_head_into_the_torso():
    d = dc.robot("fetch")[0]
    torso = d.frame_index("torso_lift_link")
    assert d.frame_mass[torso] == pytest.approx(10.7796 + 2.2556 + 0.9087 + 2 * 0.169374038216602, abs=1e-12)
    assert d.effort[d.actuated_joint_names.index("shoulder_lift_joint")] == 131.76


def test_inertial_passes_under_sanitizers(tmp_path):
    """check_inertials / fill_inertials of csrc/gto_robot.h in a stand-alone program built with AddressSanitizer and UBSan, on
    arrays of exactly the stated lengths: 1 and 32 frames, massless frames with garbage, every refusal."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "inertials"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-Wno-unknown-pragmas",
                           "-I", os.path.join(root, "grasptrajopt_amd", "csrc"), os.path.join(root, "tests", "inertials_main.cpp"),
                           "-o", str(exe)])
    rng = np.random.default_rng(4)

    def record(F, edit=None, gravity=None):
        mass, com = rng.uniform(0.1, 2.0, F), rng.uniform(-0.1, 0.1, (F, 3))
        A = rng.uniform(-0.1, 0.1, (F, 3, 3))
        I = A @ A.transpose(0, 2, 1)
        six = np.stack([I[:, 0, 0], I[:, 0, 1], I[:, 0, 2], I[:, 1, 1], I[:, 1, 2], I[:, 2, 2]], axis=1)
        if edit:
            edit(mass, com, six)
        nums = list(mass) + list(com.ravel()) + list(six.ravel()) + ([] if gravity is None else list(gravity))
        return f"{F} {int(gravity is not None)} " + " ".join(repr(float(v)) for v in nums), (mass, com, six)

    def massless(m, c, i):
        m[0], c[0], i[0] = 0.0, np.nan, -5.0

    def edit_of(k, v):
        def e(m, c, i):
            (m, c, i)[k].reshape(-1)[-1] = v
        return e

    cases = [(record(1), None), (record(32), None), (record(32, gravity=[1.0, 2.0, -3.0]), None), (record(5, massless), None),
             (record(32, edit_of(0, -1.0)), "link mass must be >= 0 and finite"),
             (record(3, edit_of(0, float("inf"))), "link mass must be >= 0 and finite"),
             (record(32, edit_of(1, float("nan"))), "non-finite centre of mass"),
             (record(2, edit_of(2, float("nan"))), "non-finite link inertia"),
             (record(32, edit_of(2, -1.0)), "link inertia must be symmetric positive semidefinite"),
             (record(4, gravity=[0.0, float("inf"), 0.0]), "non-finite gravity")]
    res = subprocess.run([str(exe)], input="\n".join(c[0][0] for c in cases), capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stderr == "", res.stdout[-2000:] + res.stderr[-4000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(cases)
    for line, ((_, (mass, com, six)), why) in zip(lines, cases):
        if why is not None:
            assert line == f"rc=-1 why={why}"
            continue
        live = mass > 0
        got = dict(kv.split("=") for kv in line.split(" gravity=")[0].split()[1:])
        assert line.startswith("rc=0 ") and float(got["mass"]) == pytest.approx(mass[live].sum(), rel=1e-14)
        assert float(got["inertia"]) == pytest.approx(six[live].sum(), rel=1e-12, abs=1e-15)
        assert float(got["com"]) == pytest.approx(com[live].sum(), rel=1e-12, abs=1e-15)
    assert lines[0].endswith("gravity=0 0 -9.8100000000000005") and lines[2].endswith("gravity=1 2 -3")


def test_exported_symbols_and_bindings():
    from grasptrajopt_amd import _capi
    assert "gto_set_link_inertials" in _capi.EXPORTED_SYMBOLS and "gto_inverse_dynamics" in _capi.EXPORTED_SYMBOLS
    assert len(_capi.PROTOTYPES["gto_inverse_dynamics"][1]) == 9 and len(_capi.PROTOTYPES["gto_set_link_inertials"][1]) == 5
    m, c, i = _capi.payload_arrays({"mass": 2.0, "com": [0, 0, 0.1]}, 3)
    assert m.tolist() == [2.0] * 3 and c.shape == (3, 3) and i is None
    m, c, i = _capi.payload_arrays({"mass": [1, 2, 3], "inertia": np.ones((3, 6))}, 3)
    assert m.tolist() == [1, 2, 3] and c is None and i.shape == (3, 6)
    assert _capi.payload_arrays(None, 4) == (None, None, None)
    for bad in ({"mass": -1.0}, {"mass": np.nan}, {"com": [0, 0, 0]}, {"mass": 1.0, "weight": 2}, {"mass": [1, 2]},
                {"mass": 1.0, "com": [0, 0]}):
        with pytest.raises(ValueError):
            _capi.payload_arrays(bad, 3)
