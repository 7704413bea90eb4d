"""OccupancyGrid — the x-y occupancy grid of the mobile pipeline (gto/gto_models.py:218-244), resident on the GPU
(gto_occupancy_*: include/gto_solver.h).

The reference's ``GTORobotModel.setup_occupancy_grid`` marks the nodes of an x-y grid that have an observed point (z > 0.01)
within ``epsilon`` and keeps the grid as a numpy array; ``BasePlanner.base_collision_cost`` then sums it under the robot's
footprint, once per draw of the driver's resampling loop (examples/pybullet_gto_planning_mobile.py:185-199).  An
``OccupancyGrid`` is that grid built on the device, from an ``Observation`` without a copy of the cloud through the host or
from host points, and kept there for ``gto_base_report_device`` (``BasePlanner.place_base``).  Its values are the reference's,
bit for bit.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import GTOError

_pd, _pi, _pu8 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


class OccupancyGrid:
    """Owns one gto_occupancy (one HIP device)."""

    def __init__(self, ptr, lib, device: int, resolution: float):
        self._g, self._lib, self.device, self.resolution = ptr, lib, device, float(resolution)
        org, shp, xl, yl = np.zeros(2), np.zeros(2, dtype=np.int32), np.zeros(2), np.zeros(2)
        self._check(lib.gto_occupancy_geometry(ptr, org.ctypes.data_as(_pd), shp.ctypes.data_as(_pi), xl.ctypes.data_as(_pd),
                                               yl.ctypes.data_as(_pd)), "gto_occupancy_geometry")
        self.origin = org.reshape((1, 2))  # as GTORobotModel.occupancy_grid_origin
        self.shape = (int(shp[0]), int(shp[1]))
        self.xlim, self.ylim = [float(xl[0]), float(xl[1])], [float(yl[0]), float(yl[1])]

    @classmethod
    def from_observation(cls, obs, margin=0.4, resolution=0.05, epsilon=0.02):
        """gto_occupancy_from_observation: the back-projected points of a depth observation or the samples of a cloud
        observation (observation.Observation, or a DepthPointCloud / SurfacePointCloud whose cached one is taken)."""
        from .observation import as_observation
        obs = as_observation(obs)
        lib = _capi.load_library()
        g = C.c_void_p()
        rc = lib.gto_occupancy_from_observation(obs._ptr(), float(margin), float(resolution), float(epsilon), C.byref(g))
        if rc != 0:
            raise GTOError(f"gto_occupancy_from_observation failed ({rc}): {lib.gto_last_error(None).decode()}")
        return cls(g, lib, obs.device, resolution)

    @classmethod
    def from_points(cls, points, margin=0.4, resolution=0.05, epsilon=0.02, device=0):
        """gto_occupancy_from_points: host points (n, 3)."""
        lib = _capi.load_library()
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        g = C.c_void_p()
        rc = lib.gto_occupancy_from_points(int(device), pts.ctypes.data_as(_pd), pts.shape[0], float(margin), float(resolution),
                                           float(epsilon), C.byref(g))
        if rc != 0:
            raise GTOError(f"gto_occupancy_from_points failed ({rc}): {lib.gto_last_error(None).decode()}")
        return cls(g, lib, int(device), resolution)

    # ------------------------------------------------------------------ lifetime
    def _ptr(self):
        if not getattr(self, "_g", None):
            raise GTOError("this OccupancyGrid is closed: its device memory was released by close()")
        return self._g

    @property
    def closed(self) -> bool:
        return not getattr(self, "_g", None)

    def close(self):
        if getattr(self, "_g", None):
            self._lib.gto_occupancy_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise GTOError(f"{what} failed ({rc}): {self._lib.gto_last_error(None).decode()}")

    # ------------------------------------------------------------------ contents
    @property
    def size(self) -> int:
        return self.shape[0] * self.shape[1]

    @property
    def grid(self):
        """The grid as uint8 (nx, ny), 0 or 1, device to host."""
        out = np.empty(self.shape, dtype=np.uint8)
        self._check(self._lib.gto_occupancy_grid(self._ptr(), out.ctypes.data_as(_pu8)), "gto_occupancy_grid")
        return out
