"""sampling/ray_sampling.rs: `shape_surface_ray_sample` / `shape_volume_ray_sample` on the device (salva_hip_sample_shape,
DESIGN.md §13).  A shape is what salva_amd.coupling.make_shape takes — ("ball", r), ("cuboid", (hx, hy, hz)), ("capsule", hh, r),
("cylinder", hh, r) — or a HostRayShape for anything else."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

F32 = np.float32
SURFACE, VOLUME = L.SAMPLE_SURFACE, L.SAMPLE_VOLUME


class HostRayShape:
    """A shape whose ray casts stay with the host (salva_hip_sample_host_shape):

      aabb() -> (mins, maxs)                          `shape.compute_aabb(&Isometry::identity())`
      cast(origins[n, 3], axis) -> toi[n]             `shape.cast_local_ray(&Ray::new(origin, e_axis), Real::MAX, false)` per ray;
                                                      a negative or NaN toi is a miss

    An exception raised in a callback is parked and re-raised by the sampling call (ctypes would swallow it): the library is handed
    a NaN box / all misses in its place."""

    def __init__(self, aabb, cast):
        self._aabb, self._cast, self._error = aabb, cast, None

        def aabb_cb(_user, mins, maxs):
            try:
                lo, hi = self._aabb()
                for a in range(3):
                    mins[a], maxs[a] = float(lo[a]), float(hi[a])
            except BaseException as e:  # noqa: BLE001
                self._error = self._error or e
                for a in range(3):
                    mins[a] = maxs[a] = float("nan")

        def cast_cb(_user, n, origins, axis, toi):
            out = np.ctypeslib.as_array(toi, shape=(n,))
            try:
                out[:] = np.asarray(self._cast(np.ctypeslib.as_array(origins, shape=(n, 3)).copy(), int(axis)), F32).reshape(n)
            except BaseException as e:  # noqa: BLE001
                self._error = self._error or e
                out[:] = -1.0

        self._thunks = (L.HOST_AABB_FN(aabb_cb), L.HOST_CAST_FN(cast_cb))
        self.shape = L.HostRayShape(None, self._thunks[0], self._thunks[1])


def _sample(shape, particle_rad: float, mode: int, world=None) -> np.ndarray:
    from .coupling import make_shape
    from .world import DFSPHSolver, LiquidWorld

    w = world if world is not None else LiquidWorld(DFSPHSolver(), float(particle_rad), 2.0)  # (supplies the device and the stream)
    fp = C.POINTER(C.c_float)
    if isinstance(shape, HostRayShape):
        def call(cap, out):
            n = w._L.salva_hip_sample_host_shape(w._h, C.byref(shape.shape), float(particle_rad), mode, cap, out)
            err, shape._error = shape._error, None
            if err is not None:
                raise err
            return n
    else:
        s = shape if isinstance(shape, L.Shape) else make_shape(shape)

        def call(cap, out):
            return w._L.salva_hip_sample_shape(w._h, C.byref(s), float(particle_rad), mode, cap, out)
    # (a host shape's casts run again with every call: a first buffer that usually suffices spares them the second pass)
    cap = 65536 if isinstance(shape, HostRayShape) else 0
    pts = np.zeros((cap, 3), F32)
    n = call(cap, pts.ctypes.data_as(fp) if cap else None)
    if n < 0:
        L.check(int(n))
    if n <= cap:
        return pts[:n].copy()
    pts = np.zeros((n, 3), F32)
    m = call(n, pts.ctypes.data_as(fp))
    if m < 0:
        L.check(int(m))
    assert m == n
    return pts


def shape_surface_ray_sample(shape, particle_rad: float, world=None) -> np.ndarray:
    """ray_sampling.rs:9-15 -> (n, 3) f32, lexicographic lattice order."""
    return _sample(shape, particle_rad, SURFACE, world)


def shape_volume_ray_sample(shape, particle_rad: float, world=None) -> np.ndarray:
    """ray_sampling.rs:18-24 -> (n, 3) f32, lexicographic lattice order."""
    return _sample(shape, particle_rad, VOLUME, world)
