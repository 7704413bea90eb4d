"""CPU: the sampled-mesh cost field's host side -- the numpy restatement against the reference's own results
(tests/golden/surface_cloud.npz), the two C entry points' declarations and argument checks, mesh placement, the object-URDF
reader and the field helpers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden
import cloud_sdf_ref as ref


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from grasptrajopt_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def spc(capi):
    from grasptrajopt_amd import surface_point_cloud
    return surface_point_cloud


@pytest.mark.parametrize("k", [11, 1])
@pytest.mark.parametrize("name", ["table", "shelf"])
def test_restatement_equals_the_reference_bit_for_bit(name, k):
    z = golden("surface_cloud.npz")
    pts, nrm = ref.unpack_cloud(z, name)
    want = z[f"{name}_sdf_k{k}"]
    mine = ref.cloud_sdf(pts, nrm, z[f"{name}_query"], k=k)
    np.testing.assert_array_equal(mine["sdf"].view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(mine["inside"], want < 0)
    # what makes bit equality a fair demand of a search that breaks ties its own way: no tie, no vote on the fence
    assert (mine["d2"][:, k - 1] != mine["d2"][:, k]).all() and (mine["dot"] != 0).all()
    assert (want < 0).any() and (want > 0).any() and want.dtype == np.float32


def test_restatement_tie_rule_prefers_the_lower_index():
    rng = np.random.default_rng(0)
    pts = rng.normal(size=(40, 3))
    pts = np.concatenate([pts, pts[::-1]])  # every sample twice
    nrm = rng.normal(size=(80, 3))
    r = ref.cloud_sdf(pts, nrm, pts[:40], k=4)
    assert (r["nearest"] == np.arange(40)).all() and (r["d2"][:, 0] == 0).all() and (r["d2"][:, 1] == 0).all()
    full = np.argsort(((pts[None] - pts[:40, None]) ** 2).sum(-1), axis=1, kind="stable")[:, :5]
    np.testing.assert_array_equal(ref.knn_rows(((pts[None, :, 0] - pts[:40, None, 0]) ** 2 + (pts[None, :, 1] - pts[:40, None, 1]) ** 2)
                                               + (pts[None, :, 2] - pts[:40, None, 2]) ** 2, 4)[:, 0], full[:, 0])


def test_get_voxels_restatement_and_raster(spc):
    z = golden("surface_cloud.npz")
    raster = spc.get_raster_points(16)
    assert raster.dtype == np.float32
    np.testing.assert_array_equal(raster, z["raster16"])
    for name in ("table", "shelf"):
        pts, nrm = ref.unpack_cloud(z, name)
        vox = ref.cloud_sdf(ref.unit_cube_cloud(pts), nrm, raster, k=11)["sdf"].reshape(16, 16, 16)
        np.testing.assert_array_equal(vox.view(np.uint32), z[f"{name}_voxels16"].view(np.uint32))


def test_header_library_and_wrapper_agree_on_the_new_calls(capi):
    hdr = open(os.path.join(ROOT, "include", "gto_solver.h")).read()
    assert int(re.search(r"#define GTO_ABI_VERSION (\d+)", hdr).group(1)) == capi.ABI_VERSION == capi.load_library().gto_version() >= 1010
    lib = capi.load_library()
    for sym in ("gto_cloud_sdf_cost", "gto_scene_from_clouds"):
        assert re.search(rf"\bint {sym}\(", hdr) and sym in capi.EXPORTED_SYMBOLS and hasattr(lib, sym)
        # each declaration cites the reference lines it replaces
        comment = hdr[:hdr.index(f"int {sym}(")].rsplit("/*", 1)[1]
        assert "surface_point_cloud.py:" in comment
    import __graft_entry__ as g
    assert "gto_cloud.h" in g.HIP_DEPS


def test_cloud_entry_point_checks_its_arguments_without_a_device(capi, spc):
    lib = capi.load_library()
    pd = C.POINTER(C.c_double)
    pts = np.random.default_rng(1).normal(size=(20, 3))
    nrm = np.tile([0.0, 0.0, 1.0], (20, 1))
    q = np.zeros((2, 3))
    p = lambda a: a.ctypes.data_as(pd)

    def call(points, normals, n, k):
        rc = lib.gto_cloud_sdf_cost(0, None if points is None else p(points), p(normals), n, k, p(q), 2, 0.02, 1.0, None, None, None, None)
        return rc, lib.gto_last_error(None).decode()

    assert call(pts, nrm, 20, 0) == (-1, "gto_cloud_sdf_cost: k must be in [1, 16]")
    assert call(pts, nrm, 20, 17) == (-1, "gto_cloud_sdf_cost: k must be in [1, 16]")
    assert call(pts, nrm, 10, 11) == (-1, "gto_cloud_sdf_cost: fewer samples than k")
    assert call(None, nrm, 20, 11) == (-1, "gto_cloud_sdf_cost: null points or normals")
    bad = pts.copy()
    bad[3, 2] = np.inf
    assert call(bad, nrm, 20, 11) == (-1, "gto_cloud_sdf_cost: non-finite point or normal")
    # the Python surface reports them as errors too, and says what is not ported
    cloud = spc.SurfacePointCloud(pts, nrm)
    with pytest.raises(capi.GTOError, match="k must be in"):
        cloud.get_sdf(q, sample_count=40)
    with pytest.raises(NotImplementedError, match="renderer"):
        cloud.get_sdf(q, use_depth_buffer=True)
    with pytest.raises(NotImplementedError, match="gradients"):
        cloud.get_sdf(q, return_gradients=True)
    with pytest.raises(NotImplementedError, match="renderer"):
        spc.get_surface_point_cloud(spc.box_mesh([1, 1, 1]), surface_point_method="scan")
    assert cloud.get_random_surface_points(7).shape == (7, 3)
    with pytest.raises(ValueError):
        spc.SurfacePointCloud(pts, nrm[:5])
    import grasptrajopt_amd
    assert grasptrajopt_amd.SurfacePointCloud is spc.SurfacePointCloud


def test_urdf_boards_land_where_the_urdf_puts_them(spc):
    z = golden("surface_cloud.npz")
    parts = spc.urdf_visual_meshes(ref.shelf_urdf_text(z["shelf_names"], z["shelf_box_size"], z["shelf_box_xyz"]))
    assert [n for n, _, _ in parts] == list(z["shelf_names"]) and len(parts) == 6
    verts = np.concatenate([v @ T[:3, :3].T + T[:3, 3] for _, (v, f), T in parts])
    faces = np.concatenate([f + 8 * i for i, (_, (v, f), T) in enumerate(parts)])
    np.testing.assert_array_equal(verts, z["shelf_vertices"])
    np.testing.assert_array_equal(faces, z["shelf_faces"])
    for (_, (v, f), T), size, xyz in zip(parts, z["shelf_box_size"], z["shelf_box_xyz"]):
        assert len(f) == 12
        np.testing.assert_allclose(v.max(0) - v.min(0), size, atol=1e-15)
        np.testing.assert_array_equal(T[:3, 3], xyz)
        np.testing.assert_allclose(spc.mesh_area(v, f), 2 * (size[0] * size[1] + size[1] * size[2] + size[0] * size[2]), rtol=1e-12)
    # the same cloud the fixture holds
    pts, nrm = spc.place_meshes([(m, T) for _, m, T in parts], counts=z["shelf_counts"], seed=2)
    want_p, want_n = ref.unpack_cloud(z, "shelf")
    np.testing.assert_array_equal(pts, want_p)
    np.testing.assert_array_equal(nrm, want_n)
    # samples lie on their board, normals point out of it
    off = 0
    for size, xyz, n in zip(z["shelf_box_size"], z["shelf_box_xyz"], z["shelf_counts"]):
        local = (pts[off:off + n] - xyz) / (size / 2)
        face_axis = np.abs(nrm[off:off + n]).argmax(axis=1)
        on = local[np.arange(n), face_axis]
        np.testing.assert_allclose(np.abs(on), 1.0, atol=1e-12)
        assert (np.sign(on) == nrm[off:off + n][np.arange(n), face_axis]).all() and (np.abs(local) <= 1 + 1e-12).all()
        off += n


def test_place_meshes_rotates_normals_with_the_pose(spc):
    c, s = np.cos(0.7), np.sin(0.7)
    pose = np.array([[c, -s, 0, 0.3], [s, c, 0, -0.2], [0, 0, 1.0, 1.5], [0, 0, 0, 1.0]])
    tilt = np.array([[1.0, 0, 0, 0], [0, 0, -1.0, 0], [0, 1.0, 0, 0], [0, 0, 0, 1.0]])
    box = spc.box_mesh([0.4, 0.2, 0.1])
    p0, n0 = spc.place_meshes([(box, np.eye(4))], counts=[500], seed=9)
    for T in (pose, pose @ tilt):
        p, n = spc.place_meshes([(box, T)], counts=[500], seed=9)
        np.testing.assert_allclose(p, p0 @ T[:3, :3].T + T[:3, 3], atol=1e-15)
        np.testing.assert_allclose(n, n0 @ T[:3, :3].T, atol=1e-15)
        np.testing.assert_allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-12)
    # density: counts follow the area; two parts are drawn with seeds of their own, in order
    pts, nrm = spc.place_meshes([(box, np.eye(4)), (box, pose)], samples_per_m2=1000.0, seed=9)
    per = int(np.ceil(1000.0 * spc.mesh_area(*box)))
    assert len(pts) == 2 * per
    np.testing.assert_array_equal(pts[:per], spc.place_meshes([(box, np.eye(4))], counts=[per], seed=9)[0])
    with pytest.raises(ValueError):
        spc.place_meshes([(box, pose)])
    # a mesh file in a URDF, scaled
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        v, f = box
        with open(os.path.join(d, "part.obj"), "w") as fh:
            fh.write("".join(f"v {float(a)!r} {float(b)!r} {float(c_)!r}\n" for a, b, c_ in v) + "".join(f"f {a + 1} {b + 1} {c_ + 1}\n" for a, b, c_ in f))
        with open(os.path.join(d, "thing.urdf"), "w") as fh:
            fh.write('<robot name="thing"><link name="base"><visual><origin xyz="0 0 1" rpy="0 0 0"/><geometry>'
                     '<mesh filename="part.obj" scale="2 2 2"/></geometry></visual></link></robot>')
        (name, (mv, mf), T), = spc.urdf_visual_meshes(os.path.join(d, "thing.urdf"))
        np.testing.assert_array_equal(mv, 2 * v)
        np.testing.assert_array_equal(T[:3, 3], [0, 0, 1])
        cloud = spc.get_surface_point_cloud(os.path.join(d, "part.obj"), sample_point_count=100, seed=3)
        assert cloud.points.shape == (100, 3)


def test_combine_cost_fields_is_the_cost_of_the_union(spc):
    rng = np.random.default_rng(4)
    da, db = rng.uniform(-0.05, 0.1, 5000), rng.uniform(-0.05, 0.1, 5000)
    for w in (1.0, 3.0):
        cost = lambda d: ref.cost_map(d.astype(np.float32), d < 0, 0.02, w)
        both = spc.combine_cost_fields(cost(da), cost(db))
        assert both.dtype == np.float32
        np.testing.assert_array_equal(both, cost(np.minimum(da, db)))
    with pytest.raises(ValueError):
        spc.combine_cost_fields(np.zeros(3), np.zeros(4))
