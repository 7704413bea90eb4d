"""CPU: the motion after the grasp.  The entry points exist in header, binding and library; the reference chain of
tests/retrieve_ref.py (a loop over the FP64 oracle) does what the contract of gto_retrieve_lift says on the inputs the GPU
tests use -- every step converges with iterations to spare, link_ee follows the line with its rotation held, limits hold,
the closed joints stay closed -- and the reversed path is the reference's index expression."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import retrieve_ref as rr
from conftest import ROOT

NEW = ("gto_retrieve_lift_device", "gto_retrieve_lift", "gto_retrieve_reverse_device", "gto_retrieve_path_columns",
       "gto_check_paths", "gto_check_paths_device")
K = 10


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


def test_new_prototypes_exist_in_header_binding_and_library(capi):
    hdr = open(os.path.join(ROOT, "include", "gto_solver.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gto_[a-z_]+)\s*\(", hdr))
    lib = capi.load_library()
    for name in NEW:
        assert name in declared, name
        assert name in capi.PROTOTYPES, name
        assert hasattr(lib, name), name
    abi = int(re.search(r"#define GTO_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "gto_solver.h")).read()).group(1))
    assert abi == capi.ABI_VERSION == lib.gto_version()
    # the lift's signature, argument by argument: 14 inputs (three of them host arrays), seven outputs, the stream
    restype, args = capi.PROTOTYPES["gto_retrieve_lift_device"]
    assert restype is C.c_int and len(args) == 22
    assert args[5] is C.POINTER(C.c_double) and args[8] is C.POINTER(C.c_int32) and args[9] is C.POINTER(C.c_double)
    assert len(capi.PROTOTYPES["gto_retrieve_lift"][1]) == 21
    assert len(capi.PROTOTYPES["gto_check_paths_device"][1]) == len(capi.PROTOTYPES["gto_check_plans_device"][1]) + 1
    for m in ("retrieve_lift", "retrieve_lift_device", "retrieve_reverse", "retrieve_path_columns", "check_paths", "check_paths_device"):
        assert callable(getattr(capi.SolverHandle, m)), m


def test_null_handles_are_refused_before_any_device_work(capi):
    lib = capi.load_library()
    z = None
    assert lib.gto_retrieve_lift_device(z, 1, z, z, z, z, 0.2, 10, z, z, 0, 50, 0.01, 5.0, z, z, z, z, z, z, z, z) == -1
    assert lib.gto_retrieve_lift(z, 1, z, z, z, z, 0.2, 10, z, z, 0, 50, 0.01, 5.0, z, z, z, z, z, z, z) == -1
    assert lib.gto_retrieve_reverse_device(z, 1, z, z, z, 0, z, z, z) == -1
    assert lib.gto_retrieve_path_columns(z) == -1
    assert lib.gto_check_paths(z, z, 0, 5, z, z, 0, z) == -1
    assert lib.gto_check_paths_device(z, z, 0, 5, z, z, 0, z, z) == -1


@pytest.fixture(scope="module", params=["panda", "fetch"])
def chain(request, oracle_mod):
    desc, cfg, plans = rr.grasp_plans(request.param, 8, seed=0)
    o = oracle_mod.Oracle(desc, cfg["link_ee"], cfg["link_gripper"], oracle_mod.reference_opts())
    closed = rr.finger_joints(desc)
    r = rr.lift_chain(o, desc, cfg["link_ee"], plans, rr.LIFT[request.param], K, closed_joints=closed, closed_values=0.0)
    return desc, cfg, plans, o, closed, r


def test_fingers_are_the_configs_finger_index(chain):
    desc, cfg, _, _, closed, _ = chain
    assert closed == list(cfg["finger_index"]) and set(closed) <= set(int(i) for i in desc.param_index)


def test_every_step_converges_with_iterations_to_spare(chain):
    r = chain[-1]
    assert (r["status"] == rr.STATUS_CONVERGED).all()
    assert r["iters"].max() <= 10 < rr.MAX_ITER, r["iters"]
    assert (r["reached"] == K).all()


def test_link_ee_follows_the_line_with_its_rotation_held(chain):
    desc, cfg, plans, o, closed, r = chain
    fe = desc.frame_index(cfg["link_ee"])
    q0 = rr.column0(plans, closed, 0.0)
    RT0 = o.eval_fk(q0)[:, fe]
    for k in range(1, K + 1):
        g = r["goals"][:, k - 1]
        assert np.array_equal(g[:, :3, :3], RT0[:, :3, :3]) and np.array_equal(g[:, 3], RT0[:, 3])
        assert np.array_equal(g[:, :2, 3], RT0[:, :2, 3])  # the direction is +z: x and y get + 0.0
        np.testing.assert_allclose(g[:, 2, 3], RT0[:, 2, 3] + rr.LIFT[desc.name] * k / K, rtol=0, atol=1e-15)
        ep, er = rr.pose_errors(g, o.eval_fk(r["path"][:, :, k])[:, fe])
        assert (ep < rr.POS_TOL).all() and (er < rr.ROT_TOL_DEG).all()
        assert np.array_equal(ep, r["err_pos"][:, k - 1]) and np.array_equal(er, r["err_rot"][:, k - 1])


def test_limits_hold_closed_joints_stay_and_column0_is_the_grasp(chain):
    desc, cfg, plans, _, closed, r = chain
    opt = np.asarray(desc.opt_index, dtype=np.int64)
    path = r["path"]
    assert (path[:, opt, 1:] >= desc.lower[opt][None, :, None]).all() and (path[:, opt, 1:] <= desc.upper[opt][None, :, None]).all()
    assert (path[:, closed, :] == 0.0).all()
    assert (plans[:, closed, -1] > 0.0).all()  # the plans end with the fingers open: closing them is the chain's doing
    rest = [d for d in range(desc.ndof) if d not in closed]
    assert np.array_equal(path[:, rest, 0], plans[:, rest, -1])
    par = [int(i) for i in desc.param_index]
    assert (path[:, par, :] == path[:, par, :1]).all()


@pytest.mark.parametrize("robot", ["panda", "fetch"])
def test_the_board_plans_converge_through_the_field_and_feel_it(robot, oracle_mod):
    desc0, cfg0, _ = rr.grasp_plans(robot, 1)
    o = oracle_mod.Oracle(desc0, cfg0["link_ee"], cfg0["link_gripper"], oracle_mod.reference_opts())
    desc, cfg, plans, scene = rr.board_case(robot, o.eval_fk)
    o.set_scene(0, *scene)
    closed = rr.finger_joints(desc)
    free = rr.lift_chain(o, desc, cfg["link_ee"], plans, rr.LIFT[robot], K, closed_joints=closed)
    r = rr.lift_chain(o, desc, cfg["link_ee"], plans, rr.LIFT[robot], K, closed_joints=closed, scene_id=0, base_pos=[0, 0, 0])
    assert (r["status"] == rr.STATUS_CONVERGED).all() and r["iters"].max() <= rr.BOARD_MAX_ITERS < rr.MAX_ITER, r["iters"]
    assert (r["reached"] == K).all()
    assert (np.abs(r["path"] - free["path"]).max(axis=(1, 2)) > 1e-2).all()  # a lifted link meets the field


@pytest.mark.parametrize("T", [50, 30])
def test_reverse_columns(T):
    rng = np.random.default_rng(T)
    plans = rng.standard_normal((3, 9, T))
    out = rr.reverse_path(plans, -10, closed_joints=[7, 8], closed_values=0.0)
    assert out.shape == (3, 9, 19)
    for i in range(19):
        assert np.array_equal(out[:, :7, i], plans[:, :7, T - 2 - i])
    assert (out[:, 7:, :] == 0.0).all()
    assert np.array_equal(out[:, :7, -1], plans[:, :7, T - 20]) and np.array_equal(out[:, :7, 0], plans[:, :7, T - 2])


def test_reverse_refuses_a_horizon_that_is_too_short():
    with pytest.raises(ValueError):
        rr.reverse_path(np.zeros((1, 9, 19)), -10)
    assert rr.reverse_path(np.zeros((1, 9, 20)), -10).shape == (1, 9, 19)
