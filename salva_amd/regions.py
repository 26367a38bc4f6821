"""Regions for `LiquidWorld.delete_particles_in` / `add_sink` (SalvaHipRegion, include/salva_hip.h): where particles
are deleted on the device.  A particle matches when its solid distance to the region is <= `margin`; `invert=True` selects the
particles that do not match (a particle with a non-finite position never matches, so an inverted region selects it)."""
from __future__ import annotations

import numpy as np

from . import _lib as L

F32 = np.float32


class Region:
    """Base of the family: `margin` (>= 0), `invert`, and `_struct(world)`, the SalvaHipRegion the library reads."""

    kind = 0

    def __init__(self, margin: float = 0.0, invert: bool = False):
        self.margin, self.invert = float(margin), bool(invert)

    def _fill(self, r: "L.Region", world):
        raise NotImplementedError

    def _struct(self, world) -> "L.Region":
        r = L.Region()
        r.struct_size, r.version = L.REGION_BYTES, L.REGION_VERSION
        r.kind, r.flags, r.margin = self.kind, (L.REGION_INVERT if self.invert else 0), self.margin
        r.rotation_ijkw[3] = 1.0
        self._fill(r, world)
        return r


class HalfSpace(Region):
    """Everything behind the plane through `point` with outward unit `normal`: d = normal . (x - point)."""

    kind = L.REGION_HALFSPACE

    def __init__(self, point, normal, margin: float = 0.0, invert: bool = False):
        super().__init__(margin, invert)
        self.point, self.normal = np.asarray(point, F32).reshape(3), np.asarray(normal, F32).reshape(3)

    def _fill(self, r, world):
        r.point[:], r.normal[:] = [float(x) for x in self.point], [float(x) for x in self.normal]


class Aabb(Region):
    """The box [mins, maxs]."""

    kind = L.REGION_AABB

    def __init__(self, mins, maxs, margin: float = 0.0, invert: bool = False):
        super().__init__(margin, invert)
        self.mins, self.maxs = np.asarray(mins, F32).reshape(3), np.asarray(maxs, F32).reshape(3)

    def _fill(self, r, world):
        r.mins[:], r.maxs[:] = [float(x) for x in self.mins], [float(x) for x in self.maxs]


class _Posed(Region):
    def __init__(self, translation, rotation, margin, invert):
        super().__init__(margin, invert)
        self.translation, self.rotation = np.asarray(translation, F32).reshape(3), np.asarray(rotation, F32).reshape(4)

    def _fill(self, r, world):
        r.translation[:], r.rotation_ijkw[:] = [float(x) for x in self.translation], [float(x) for x in self.rotation]


class Shape(_Posed):
    """A posed built-in shape: what coupling.make_shape takes — ("ball", r), ("cuboid", half_extents), ("capsule", hh, r),
    ("cylinder", hh, r) — or an L.Shape."""

    kind = L.REGION_SHAPE

    def __init__(self, shape, translation=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.0, 1.0), margin: float = 0.0, invert: bool = False):
        from .coupling import make_shape

        super().__init__(translation, rotation, margin, invert)
        self.shape = shape if isinstance(shape, L.Shape) else make_shape(shape)

    def _fill(self, r, world):
        super()._fill(r, world)
        r.shape.kind = self.shape.kind
        r.shape.params[:] = list(self.shape.params)


class Mesh(_Posed):
    """A posed oriented sampling.Mesh."""

    kind = L.REGION_MESH

    def __init__(self, mesh, translation=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.0, 1.0), margin: float = 0.0, invert: bool = False):
        super().__init__(translation, rotation, margin, invert)
        self.mesh = mesh

    def _fill(self, r, world):
        super()._fill(r, world)
        r.handle = self.mesh.handle(world)


class Compound(_Posed):
    """A posed sampling.Compound whose mesh parts are all oriented."""

    kind = L.REGION_COMPOUND

    def __init__(self, compound, translation=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.0, 1.0), margin: float = 0.0, invert: bool = False):
        super().__init__(translation, rotation, margin, invert)
        self.compound = compound

    def _fill(self, r, world):
        super()._fill(r, world)
        r.handle = self.compound.handle(world)
