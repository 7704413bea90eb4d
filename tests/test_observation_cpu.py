"""CPU: the resident observation's C ABI (declared, exported, bound with matching argument types), its argument checks ahead
of the device check, and the collision fixture tests/golden/collision_checks.npz (made by tests/golden/make_collision_golden.py
from the reference's own DepthPointCloud and its two collision loops).

The create calls validate before they look for a device (as gto_depth_sdf_cost and gto_cloud_sdf_cost do): without a GPU a
valid input ends in GTO_ERR_NO_DEVICE (-3), an invalid one in GTO_ERR_INVALID_ARG (-1).  With a GPU the valid input is
created and destroyed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden
from grasptrajopt_amd import _capi

NEW_SYMBOLS = ("gto_observation_from_depth", "gto_observation_from_cloud", "gto_observation_destroy", "gto_observation_sdf",
               "gto_observation_check_posed", "gto_check_plans", "gto_check_plans_device")

_pd, _pf, _pi, _pu8 = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
CTYPE = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "float": C.c_float,
         "const float*": _pf, "float*": _pf, "const double*": _pd, "double*": _pd, "const uint8_t*": _pu8, "uint8_t*": _pu8,
         "int32_t*": _pi, "const int32_t*": _pi, "gto_observation*": C.c_void_p, "gto_handle*": C.c_void_p, "void*": C.c_void_p,
         "gto_observation**": C.POINTER(C.c_void_p)}


def header_signature(name):
    """(return type, [argument types]) of a function declared in include/gto_solver.h."""
    text = open(os.path.join(ROOT, "include", "gto_solver.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\b(int|void)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/gto_solver.h"
    args = []
    for a in m.group(2).split(","):
        a = " ".join(a.split())
        typ = re.sub(r"\s*\b\w+$", "", a) if not a.endswith("*") else a  # drop the parameter name
        args.append(typ.replace(" *", "*").replace("* ", "*"))
    return m.group(1), args


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_symbol_is_declared_exported_and_bound(name):
    ret, args = header_signature(name)
    lib = _capi.load_library()
    assert name in _capi.EXPORTED_SYMBOLS
    fn = getattr(lib, name)  # exported by the library
    assert fn.restype == (None if ret == "void" else C.c_int)
    want = [CTYPE[a] for a in args]
    # device pointers travel as void pointers in the binding (ints from torch.Tensor.data_ptr())
    if name == "gto_check_plans_device":
        want[3], want[6] = C.c_void_p, C.c_void_p
    assert list(fn.argtypes) == want, f"{name}: header {args}, binding {fn.argtypes}"


def test_abi_version_moves_with_the_header():
    text = open(os.path.join(ROOT, "include", "gto_solver.h")).read()
    v = int(re.search(r"#define GTO_ABI_VERSION (\d+)", text).group(1))
    assert v == _capi.ABI_VERSION == int(_capi.load_library().gto_version()) and v >= 1011


def _depth_args(H=6, W=8):
    depth = np.ones((max(H, 1), max(W, 1)), dtype=np.float32)
    K, cam = np.eye(3), np.eye(4)
    return depth, K, cam


def _from_depth(lib, H, W, depth=True):
    d, K, cam = _depth_args(H, W)
    o = C.c_void_p()
    rc = lib.gto_observation_from_depth(0, d.ctypes.data_as(_pf) if depth else None, H, W, K.ctypes.data_as(_pd), K.ctypes.data_as(_pd),
                                        cam.ctypes.data_as(_pd), cam.ctypes.data_as(_pd), None, 1.5, C.byref(o))
    return rc, o


def _from_cloud(lib, n, k):
    rng = np.random.default_rng(0)
    pts, nrm = rng.normal(size=(max(n, 1), 3)), rng.normal(size=(max(n, 1), 3))
    o = C.c_void_p()
    rc = lib.gto_observation_from_cloud(0, pts.ctypes.data_as(_pd), nrm.ctypes.data_as(_pd), n, k, C.byref(o))
    return rc, o


def test_create_validates_before_it_looks_for_a_device():
    lib = _capi.load_library()
    for H, W in ((0, 8), (6, 0), (-1, 8)):
        rc, o = _from_depth(lib, H, W)
        assert rc == -1 and not o.value and b"gto_observation_from_depth" in lib.gto_last_error(None)
    rc, o = _from_depth(lib, 6, 8, depth=False)
    assert rc == -1 and not o.value
    for n, k, why in ((5, 11, b"fewer samples than k"), (40, 0, b"k must be in [1, 16]"), (40, 17, b"k must be in [1, 16]")):
        rc, o = _from_cloud(lib, n, k)
        assert rc == -1 and not o.value and why in lib.gto_last_error(None), (n, k, lib.gto_last_error(None))
    # k is checked before n, as gto_cloud_sdf_cost checks them
    rc, o = _from_cloud(lib, 5, 17)
    assert rc == -1 and b"k must be in [1, 16]" in lib.gto_last_error(None)
    # valid inputs: no device -> GTO_ERR_NO_DEVICE; with one they are created
    for rc, o in (_from_depth(lib, 6, 8), _from_cloud(lib, 40, 11)):
        assert rc in (0, -3)
        if rc == 0:
            assert o.value
            lib.gto_observation_destroy(o)
        else:
            assert not o.value and b"no HIP device" in lib.gto_last_error(None)
    lib.gto_observation_destroy(None)  # a null observation is ignored


def test_queries_refuse_a_null_observation():
    lib = _capi.load_library()
    q = np.zeros((2, 3))
    cnt = np.zeros(2, dtype=np.int32)
    assert lib.gto_observation_sdf(None, q.ctypes.data_as(_pd), 2, None, None) == -1
    assert lib.gto_observation_check_posed(None, q.ctypes.data_as(_pd), 2, np.zeros((2, 16)).ctypes.data_as(_pd), 2, cnt.ctypes.data_as(_pi)) == -1
    assert lib.gto_check_plans(None, None, 0, None, None, 0, None) == -1


def test_closed_observation_names_the_cause():
    from grasptrajopt_amd.observation import Observation
    o = Observation(None, _capi.load_library(), "depth", 0)
    assert o.closed
    with pytest.raises(_capi.GTOError, match="closed"):
        o.sdf(np.zeros((1, 3)))
    with pytest.raises(_capi.GTOError, match="closed"):
        o.check_posed(np.zeros((1, 3)), np.eye(4)[None])
    o.close()  # closing twice is harmless


def test_collision_fixture_is_not_trivial():
    z = golden("collision_checks.npz")
    plans, counts = z["plans"], z["plan_counts"]
    B, ndof, T = plans.shape
    assert z["depth"].shape == (120, 160) and z["depth"].dtype == np.float32 and counts.shape == (B, T) and ndof == 9
    hit = (counts > 5).any(axis=1)
    np.testing.assert_array_equal(hit, z["plan_in_collision"])
    assert hit.sum() >= B / 4 and (~hit).sum() >= B / 4
    assert ((counts >= 1) & (counts <= 5)).any() and (counts > 5).any()
    P = z["gripper_points"].shape[0]
    ratio = z["grasp_counts"] / P
    assert (ratio > 0.01).any() and (ratio <= 0.01).any()
    np.testing.assert_array_equal((ratio > 0.01).astype(np.int32), z["grasp_in_collision"])
    # no query of the generator coincided with a cloud point (there the reference's -0 is not "< 0" and the counts would differ)
    assert float(z["plan_min_abs_sdf"]) > 0 and float(z["grasp_min_abs_sdf"]) > 0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "collision_checks.npz")) < (1 << 20)
    assert np.isfinite(plans).all() and np.isfinite(z["poses"]).all()


def test_numpy_einsum_adds_the_products_in_the_order_the_posed_kernel_copies():
    """utils.grasp_collision_ratio places the gripper's points with numpy.einsum("nij,pj->npi"); k_check_posed (gto_observe.h)
    copies the order in which this numpy adds the three products of a row, (R_i0 p_0 + R_i2 p_2) + R_i1 p_1, so that both
    place the same bits.  The order is numpy's own business: if a numpy release changes it, this test says so here, without a
    GPU, and the kernel's order has to follow."""
    rng = np.random.default_rng(3)
    for n, P in ((1, 1), (1, 1200), (64, 300), (7, 13), (200, 5004)):
        RT = rng.normal(size=(n, 4, 4))
        pts = rng.normal(size=(P, 3))
        R = RT[:, :3, :3]  # the slice grasp_collision_ratio passes
        got = np.einsum("nij,pj->npi", R, pts)
        pr = [R[:, None, :, j] * pts[None, :, None, j] for j in range(3)]
        np.testing.assert_array_equal(got, (pr[0] + pr[2]) + pr[1])
