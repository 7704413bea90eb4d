"""SurfacePointCloud — drop-in for the reference's mesh_to_sdf/surface_point_cloud.py, for scenes whose
geometry is known as triangle meshes.

The reference keeps a sampled mesh (points + face normals) in a scikit-learn KD-tree and answers ``get_sdf`` with the
distance to the nearest sample, signed by a vote of the normals of the ``sample_count = 11`` nearest samples
(mesh_to_sdf/surface_point_cloud.py:32-64, the ``use_depth_buffer=False`` branch that ``mesh_to_sdf(...,
surface_point_method='sample')`` takes).  Here the k-nearest-neighbour search (FP64, a bounding-box hierarchy over the
Morton-sorted samples walked by packets of 64 neighbouring queries), the vote and the cost map run in
``gto_cloud_sdf_cost``; the values are bit-identical to the reference wherever the k-th and (k+1)-th neighbour are not
at the same distance (tests/golden/surface_cloud.npz).  An instance can stand wherever a ``DepthPointCloud`` does:
``get_sdf`` for ``utils.plan_in_collision`` / ``utils.grasp_collision_ratio``, ``get_sdf_cost`` for the planner's and the
IK solver's fields; ``GTORobotModel.setup_clouds_field`` leaves both fields resident on the device.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _capi
from .depth_scene import LazyCostField, Resident
from .mesh import load_mesh, sample_surface

MAX_SAMPLE_COUNT = 16  # GTO_CLOUD_MAX_K (csrc/gto_cloud.h)


def get_raster_points(voxel_resolution):
    """mesh_to_sdf/utils.py:26-34: the float32 centres of a voxel_resolution^3 raster of [-1, 1]^3, x slowest."""
    ax = np.linspace(-1, 1, voxel_resolution)
    points = np.stack(np.meshgrid(ax, ax, ax))
    points = np.swapaxes(points, 1, 2)
    return points.reshape(3, -1).transpose().astype(np.float32)


class SurfacePointCloud:
    def __init__(self, points, normals, device=0):
        self.points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        self.normals = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
        if self.points.shape != self.normals.shape:
            raise ValueError("points and normals must have the same shape")
        self.device = device
        self._lib = _capi.load_library()

    # ------------------------------------------------------------------ the one GPU call
    def _run(self, query, sample_count=11, epsilon=0.02, w_inside=1.0):
        """(sdf float32, inside bool, cost float32, nearest int32) of the query points."""
        query = np.ascontiguousarray(query, dtype=np.float64).reshape(-1, 3)
        nq = query.shape[0]
        sdf, cost = np.empty(nq, dtype=np.float32), np.empty(nq, dtype=np.float32)
        inside, nearest = np.empty(nq, dtype=np.uint8), np.empty(nq, dtype=np.int32)
        pu8, pf, pd, pi = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
        rc = self._lib.gto_cloud_sdf_cost(self.device, self.points.ctypes.data_as(pd), self.normals.ctypes.data_as(pd),
                                          self.points.shape[0], int(sample_count), query.ctypes.data_as(pd), nq, float(epsilon),
                                          float(w_inside), sdf.ctypes.data_as(pf), inside.ctypes.data_as(pu8),
                                          cost.ctypes.data_as(pf), nearest.ctypes.data_as(pi))
        if rc != 0:
            raise _capi.GTOError(f"gto_cloud_sdf_cost failed ({rc}): {self._lib.gto_last_error(None).decode()}")
        return sdf, inside.astype(bool), cost, nearest

    # ------------------------------------------------------------------ reference surface
    def get_random_surface_points(self, count, use_scans=True):
        """:24-30 (there is no mesh to sample anew: the stored samples are drawn from, as with use_scans=True)."""
        indices = np.random.choice(self.points.shape[0], count)
        return self.points[indices, :]

    def get_sdf(self, query_points, use_depth_buffer=False, sample_count=11, return_gradients=False):
        """:32-64 — float32 signed distances."""
        if use_depth_buffer:
            raise NotImplementedError("get_sdf(use_depth_buffer=True) needs the scans of an OpenGL renderer, which are not ported")
        if return_gradients:
            raise NotImplementedError("get_sdf(return_gradients=True): SDF gradients are unused by the planning path and not ported")
        return self._run(query_points, sample_count)[0]

    def get_sdf_cost(self, query_points, epsilon=0.02, w_inside=1, vis=False, sample_count=11):
        """DepthPointCloud.get_sdf_cost's signature (mesh_to_sdf/depth_point_cloud.py:64-91) over this cloud's signed
        distances: float32 costs (``vis`` is ignored: no viewer here)."""
        return self._run(query_points, sample_count, epsilon, w_inside)[2]

    def get_sdf_in_batches(self, query_points, use_depth_buffer=False, sample_count=11, batch_size=1000000, return_gradients=False):
        """:66-81."""
        query_points = np.asarray(query_points)
        if query_points.shape[0] <= batch_size:
            return self.get_sdf(query_points, use_depth_buffer, sample_count, return_gradients)
        n_batches = int(math.ceil(query_points.shape[0] / batch_size))
        return np.concatenate([self.get_sdf(pts, use_depth_buffer, sample_count, return_gradients)
                               for pts in np.array_split(query_points, n_batches)])

    def get_voxels(self, voxel_resolution, use_depth_buffer=False, sample_count=11, pad=False, check_result=False,
                   return_gradients=False):
        """:83-105 without check_result's BadMeshException."""
        if check_result:
            raise NotImplementedError("get_voxels(check_result=True) is not ported")
        sdf = self.get_sdf_in_batches(get_raster_points(voxel_resolution), use_depth_buffer, sample_count,
                                      return_gradients=return_gradients)
        voxels = sdf.reshape((voxel_resolution, voxel_resolution, voxel_resolution))
        if pad:
            voxels = np.pad(voxels, 1, mode="constant", constant_values=1)
        return voxels

    def observation(self, sample_count=11):
        """This cloud resident on the device (observation.Observation) for the vote of ``sample_count`` neighbours, built on
        first use and kept: samples, normals and their hierarchy stay there for sdf / check_posed / check_plans."""
        from .observation import Observation
        cache = self.__dict__.setdefault("_observations", {})
        o = cache.get(int(sample_count))
        if o is None or o.closed:
            o = cache[int(sample_count)] = Observation.from_cloud(self.points, self.normals, int(sample_count), self.device)
        return o

    def nearest_sample(self, query_points, sample_count=11):
        """Index of the nearest sample of every query (the lower index among samples at equal distance)."""
        return self._run(query_points, sample_count)[3]


# ---------------------------------------------------------------------- clouds from meshes
def _as_mesh(mesh):
    """(vertices (V, 3) f64, faces (F, 3) i64) of a pair or of a path mesh.load_mesh reads."""
    if isinstance(mesh, (str, os.PathLike)):
        return load_mesh(os.fspath(mesh))
    v, f = mesh
    return np.asarray(v, dtype=np.float64).reshape(-1, 3), np.asarray(f, dtype=np.int64).reshape(-1, 3)


def get_surface_point_cloud(mesh, surface_point_method="sample", sample_point_count=10000000, seed=0, device=0):
    """mesh_to_sdf/__init__.py:7-22 for surface_point_method='sample' (surface_point_cloud.py:177-188), seeded."""
    if surface_point_method != "sample":
        raise NotImplementedError(f"surface_point_method={surface_point_method!r} needs an OpenGL renderer; only 'sample' is ported")
    v, f = _as_mesh(mesh)
    pts, nrm = sample_surface(v, f, int(sample_point_count), seed=seed)
    return SurfacePointCloud(pts, nrm, device=device)


def mesh_to_sdf(mesh, query_points, surface_point_method="sample", sign_method="normal", sample_point_count=10000000,
                normal_sample_count=11, seed=0, device=0):
    """mesh_to_sdf/__init__.py:24-42 on the 'sample' / 'normal' path."""
    if not isinstance(query_points, np.ndarray):
        raise TypeError("query_points must be a numpy array.")
    if len(query_points.shape) != 2 or query_points.shape[1] != 3:
        raise ValueError("query_points must be of shape N x 3.")
    if sign_method != "normal":
        raise NotImplementedError("sign_method='depth' needs an OpenGL renderer; only 'normal' is ported")
    cloud = get_surface_point_cloud(mesh, surface_point_method, sample_point_count, seed, device)
    return cloud.get_sdf_in_batches(query_points, use_depth_buffer=False, sample_count=normal_sample_count)


def box_mesh(size):
    """The 12 triangles of an axis-aligned box of the given edge lengths about the origin, normals outward."""
    h = np.asarray(size, dtype=np.float64).reshape(3) / 2.0
    v = np.array([[sx * h[0], sy * h[1], sz * h[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5],    # -x, +x
                  [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],    # -y, +y
                  [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], dtype=np.int64)  # -z, +z
    return v, f


def mesh_area(vertices, faces):
    a = vertices[faces[:, 0]]
    return 0.5 * np.linalg.norm(np.cross(vertices[faces[:, 1]] - a, vertices[faces[:, 2]] - a), axis=1).sum()


def place_meshes(parts, samples_per_m2=None, counts=None, seed=0):
    """One cloud for furniture made of parts: ``parts`` = [(mesh, 4x4 pose), ...] (mesh: (vertices, faces) or a path).
    Part i gets ``counts[i]`` samples, or ``ceil(samples_per_m2 * its area)``, drawn with seed ``seed + i``; points are
    moved and normals rotated by the part's pose.  Returns (points (N, 3), normals (N, 3)), parts in order."""
    if (samples_per_m2 is None) == (counts is None):
        raise ValueError("give exactly one of samples_per_m2 and counts")
    pts_all, nrm_all = [], []
    for i, (mesh, pose) in enumerate(parts):
        v, f = _as_mesh(mesh)
        pose = np.asarray(pose, dtype=np.float64).reshape(4, 4)
        n = int(counts[i]) if counts is not None else int(math.ceil(samples_per_m2 * mesh_area(v, f)))
        p, nr = sample_surface(v, f, n, seed=seed + i)
        pts_all.append(p @ pose[:3, :3].T + pose[:3, 3])
        nrm_all.append(nr @ pose[:3, :3].T)
    return np.concatenate(pts_all), np.concatenate(nrm_all)


def _pose(xyz, rpy):
    from .gto_models import _rpy2r
    T = np.eye(4)
    T[:3, :3] = _rpy2r(rpy)
    T[:3, 3] = xyz
    return T


def urdf_visual_meshes(urdf, base_pose=None):
    """The visuals of an object URDF (a file name, URDF text or a urdf.Urdf) as [(link name, mesh, 4x4 pose), ...] in the
    frame of its root link (or ``base_pose``): every link's FIRST <visual>, a <box> as its 12 triangles, a <mesh> read by
    mesh.load_mesh relative to the URDF's directory and scaled.  Joints are taken at their origins (object URDFs are
    rigid: fixed joints)."""
    from .urdf import Urdf
    where = "."
    if isinstance(urdf, Urdf):
        model = urdf
    elif isinstance(urdf, str) and urdf.lstrip().startswith("<"):
        model = Urdf.from_string(urdf)
    else:
        model, where = Urdf.from_file(os.fspath(urdf)), os.path.dirname(os.path.abspath(os.fspath(urdf)))
    root = model.get_root()
    base = np.eye(4) if base_pose is None else np.asarray(base_pose, dtype=np.float64).reshape(4, 4)
    out = []
    for link in model.links:
        if not link.has_visual:
            continue
        T = np.eye(4)
        for jname in model.get_chain(root, link.name):
            j = model.joint_map[jname]
            T = T @ _pose(j.xyz, j.rpy)
        T = base @ T @ _pose(link.visual_xyz, link.visual_rpy)
        if link.visual_box is not None:
            mesh = box_mesh(link.visual_box)
        elif link.visual_mesh is not None:
            v, f = load_mesh(os.path.join(where, link.visual_mesh))
            mesh = (v * np.asarray(link.visual_scale, dtype=np.float64), f)
        else:
            continue
        out.append((link.name, mesh, T))
    return out


# ---------------------------------------------------------------------- fields
def combine_cost_fields(a, b):
    """Cost field of the union of two sets of obstacles on the same grid: the element-wise maximum.  The cost map
    (mesh_to_sdf/depth_point_cloud.py:84-89) is non-increasing in the signed distance for w_inside >= 1, and the signed
    distance to a union is the minimum of the two, so the maximum of the costs is the cost of the union: a mesh shelf and a
    depth-seen clutter can be planned against together.  Returns a float32 array (resident fields come to the host)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if a.shape != b.shape:
        raise ValueError(f"fields of different grids: {a.shape} and {b.shape}")
    return np.maximum(a, b)


class ResidentCloudField(LazyCostField):
    """A cost field that GTORobotModel.setup_clouds_field left resident: field `half` of scene `sid` of `handle`.  The planner,
    the IK solver and compute_plan_cost read it where it is (depth_scene.resident_of); anything that treats it as an array
    gets the float32 array.  It stands for that build of the scene only: after the scene is rebuilt it refuses."""

    def __init__(self, robot, where: Resident):
        self.robot, self._where = robot, where

    def resident(self):
        w = self._where
        return None if self._edited or w.gen != w.handle.scene_generation(w.sid) else w

    def _materialize(self):
        w = self._where
        if w.gen != w.handle.scene_generation(w.sid):
            raise RuntimeError("the resident scene this cost field belongs to has been rebuilt: call setup_clouds_field again")
        return w.handle.scene_fields(w.sid)[w.half]
