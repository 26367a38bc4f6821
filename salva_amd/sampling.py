"""sampling/ray_sampling.rs: `shape_surface_ray_sample` / `shape_volume_ray_sample` on the device (salva_hip_sample_shape,
DESIGN.md §13).  A shape is what salva_amd.coupling.make_shape takes — ("ball", r), ("cuboid", (hx, hy, hz)), ("capsule", hh, r),
("cylinder", hh, r) — a Mesh (triangle mesh or height field, cast at on the device: DESIGN.md §14), a Compound of such parts
(DESIGN.md §17), or a HostRayShape for anything else."""
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


class Mesh:
    """A triangle mesh (parry `TriMesh`) or, through `Mesh.heightfield`, a height field (parry `HeightField`) that lives on the
    device (salva_hip_create_mesh / salva_hip_create_heightfield).  `oriented=True` states that the mesh is closed and wound
    counter-clockwise seen from outside: only such a mesh has an inside for DynamicContactSampling to push particles out of.
    Accepted wherever a shape is: shape_surface_ray_sample / shape_volume_ray_sample, Fluid.add_particles_from_shape,
    StaticSampling.from_shape and DynamicContactSampling.  The device copy belongs to a world and is made on first use there."""

    def __init__(self, vertices, indices, oriented: bool = False):
        self.vertices = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
        self.indices = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
        self.oriented = bool(oriented)
        self._heights = self._scale = None

    @classmethod
    def heightfield(cls, heights, scale) -> "Mesh":
        """parry `HeightField::new(heights, scale)`: heights[i][j] over a grid of `scale[0]` x `scale[2]` centred at the origin,
        rows along z, columns along x, two triangles per cell."""
        self = cls(np.zeros((0, 3), F32), np.zeros((0, 3), np.uint32))
        self._heights = np.ascontiguousarray(heights, F32)
        if self._heights.ndim != 2:
            raise ValueError("heights: a 2D array, rows along z")
        self._scale = np.ascontiguousarray(scale, F32).reshape(3)
        return self

    def handle(self, world) -> int:
        """The mesh's handle in `world`, created on first use."""
        table = world.__dict__.setdefault("_mesh_handles", {})
        hit = table.get(id(self))
        if hit is not None:
            return hit[1]
        h = C.c_uint32()
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        if self._heights is not None:
            L.check(world._L.salva_hip_create_heightfield(world._h, self._heights.ctypes.data_as(fp), self._heights.shape[0],
                                                          self._heights.shape[1], self._scale.ctypes.data_as(fp), C.byref(h)))
        else:
            L.check(world._L.salva_hip_create_mesh(world._h, self.vertices.ctypes.data_as(fp), len(self.vertices),
                                                   self.indices.ctypes.data_as(up), len(self.indices),
                                                   L.MESH_ORIENTED if self.oriented else 0, C.byref(h)))
        table[id(self)] = (self, h.value)  # (keeps the mesh alive, so that its id stays its own)
        return h.value

    def destroy(self, world):
        """salva_hip_destroy_mesh: refused while a dynamically sampled boundary of `world` still uses the mesh."""
        table = world.__dict__.get("_mesh_handles", {})
        hit = table.get(id(self))
        if hit is not None:
            L.check(world._L.salva_hip_destroy_mesh(world._h, hit[1]))
            del table[id(self)]


class Compound:
    """parry's `Compound` on the device (salva_hip_create_compound): `parts` is a list of (shape, translation,
    rotation) with `shape` anything coupling.make_shape accepts or a Mesh, and (translation, unit quaternion (i, j, k, w)) the
    part's pose in the compound's frame.  Accepted wherever a shape is: shape_surface_ray_sample / shape_volume_ray_sample (one
    thread per ray casts at every part in the part's frame: salva_hip_sample_compound), Fluid.add_particles_from_shape,
    StaticSampling.from_shape, DynamicContactSampling and LiquidWorld.particles_intersecting_shape.  The device copy belongs to a
    world and is made on first use there."""

    def __init__(self, parts):
        from .coupling import make_shape

        self.parts = []
        for shape, translation, rotation in parts:
            s = shape if isinstance(shape, (L.Shape, Mesh)) else make_shape(shape)
            self.parts.append((s, np.ascontiguousarray(translation, F32).reshape(3), np.ascontiguousarray(rotation, F32).reshape(4)))

    def handle(self, world) -> int:
        """The compound's handle in `world`, created on first use (its meshes' handles with it)."""
        table = world.__dict__.setdefault("_compound_handles", {})
        hit = table.get(id(self))
        if hit is not None:
            return hit[1]
        arr = (L.CompoundPart * max(len(self.parts), 1))()
        for k, (s, t, q) in enumerate(self.parts):
            if isinstance(s, Mesh):
                arr[k].kind, arr[k].mesh = L.SHAPE_MESH, s.handle(world)
            else:
                arr[k].kind = s.kind
                arr[k].params[:] = list(s.params)
            arr[k].translation[:] = [float(x) for x in t]
            arr[k].rotation_ijkw[:] = [float(x) for x in q]
        h = C.c_uint32()
        L.check(world._L.salva_hip_create_compound(world._h, arr, len(self.parts), C.byref(h)))
        table[id(self)] = (self, h.value)  # (keeps the compound alive, so that its id stays its own)
        return h.value

    def destroy(self, world):
        """salva_hip_destroy_compound: refused while a dynamically sampled boundary of `world` still uses the compound."""
        table = world.__dict__.get("_compound_handles", {})
        hit = table.get(id(self))
        if hit is not None:
            L.check(world._L.salva_hip_destroy_compound(world._h, hit[1]))
            del table[id(self)]


# the entry that takes a built-in SalvaHipShape, where its name is not `salva_hip_<family>_shape`
_SHAPE_ENTRY = {"add_particles_sampled": "salva_hip_add_particles_sampled",
                "set_boundary_dynamic_sampling": "salva_hip_set_boundary_dynamic_sampling"}


def geometry_entry(world, family: str, shape):
    """The one place that knows the forms a geometry takes: -> (entry point of `family` for `shape`, its geometry
    argument).  `family` is "sample", "add_particles_sampled", "set_boundary_sampling_from", "set_boundary_dynamic_sampling" or
    "particles_intersecting"; `shape` is a Mesh or a Compound (the argument is its handle in `world`, created on first use), a
    HostRayShape where the family has a host entry (sampling only), or what coupling.make_shape takes."""
    from .coupling import make_shape

    for cls, form in ((Mesh, "mesh"), (Compound, "compound")):
        if isinstance(shape, cls):
            return getattr(world._L, f"salva_hip_{family}_{form}"), shape.handle(world)
    if isinstance(shape, HostRayShape) and family == "sample":
        return world._L.salva_hip_sample_host_shape, C.byref(shape.shape)
    s = shape if isinstance(shape, L.Shape) else make_shape(shape)
    return getattr(world._L, _SHAPE_ENTRY.get(family, f"salva_hip_{family}_shape")), C.byref(s)


def _sample(shape, particle_rad: float, mode: int, world=None) -> np.ndarray:
    from .world import DFSPHSolver, LiquidWorld

    w = world if world is not None else LiquidWorld(DFSPHSolver(), float(particle_rad), 2.0)  # (supplies the device and the stream)
    fp = C.POINTER(C.c_float)
    entry, geom = geometry_entry(w, "sample", shape)

    def call(cap, out):
        n = entry(w._h, geom, float(particle_rad), mode, cap, out)
        err = getattr(shape, "_error", None)  # (a HostRayShape's callbacks park their exceptions)
        if err is not None:
            shape._error = None
            raise err
        return n
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
