"""Diffuse particles - spray, foam and bubbles after Ihmsen et al. 2012 (include/salva_hip.h "Diffuse particles"): the
parameters, the potentials read out per particle on the device (LiquidWorld.diffuse_potentials), and a set of diffuse particles that
lives on the device (LiquidWorld.create_diffuse)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib as L

F32 = np.float32


@dataclass
class Diffuse:
    """SalvaHipDiffuse; the defaults are salva_hip_default_diffuse's."""
    surface_min: float = 0.25   # a particle has a normal when h |g| reaches this
    crest_cos: float = 0.6      # a crest moves along its normal at least this much
    trapped_air: Tuple[float, float] = (5.0, 20.0)   # the clamp ranges (lo, hi) of the three potentials
    wave_crest: Tuple[float, float] = (2.0, 8.0)
    energy: Tuple[float, float] = (5.0, 50.0)
    k_ta: float = 4000.0        # particles per unit of time at full potential
    k_wc: float = 50000.0
    max_per_particle: int = 16
    n_spray: int = 6            # spray below, bubble above n_bubble fluid neighbours, foam between
    n_bubble: int = 20
    k_b: float = 2.0            # buoyancy
    k_d: float = 0.8            # drag
    lifetime: Tuple[float, float] = (2.0, 5.0)
    seed: int = 0
    kill_box: Optional[Tuple[Sequence[float], Sequence[float]]] = None  # (lo, hi)
    gravity: Tuple[float, float, float] = (0.0, -9.81, 0.0)  # what the world is stepped with

    def _struct(self):
        p = L.DiffuseParams()
        p.struct_size, p.version = L.DIFFUSE_BYTES, L.DIFFUSE_VERSION
        p.surface_min, p.crest_cos = float(self.surface_min), float(self.crest_cos)
        (p.ta_lo, p.ta_hi), (p.wc_lo, p.wc_hi), (p.en_lo, p.en_hi) = map(float, self.trapped_air), map(float, self.wave_crest), map(float, self.energy)
        p.k_ta, p.k_wc, p.max_per_particle = float(self.k_ta), float(self.k_wc), int(self.max_per_particle)
        p.n_spray, p.n_bubble, p.k_b, p.k_d = int(self.n_spray), int(self.n_bubble), float(self.k_b), float(self.k_d)
        (p.life_lo, p.life_hi), p.seed = map(float, self.lifetime), int(self.seed) & 0xFFFFFFFF
        if self.kill_box is not None:
            p.has_kill_box = 1
            for a in range(3):
                p.kill_lo[a], p.kill_hi[a] = float(self.kill_box[0][a]), float(self.kill_box[1][a])
        for a in range(3):
            p.gravity[a] = float(self.gravity[a])
        return p


POTENTIALS = {"trapped_air": 1, "wave_crest": 1, "energy": 1, "normal": 3, "count": 1}  # words per row


def potentials(world, params=None, fluids=None, **which):
    """LiquidWorld.diffuse_potentials: a dict of numpy arrays, rows by fluid slot, then by index.  `which`: trapped_air= / wave_crest=
    / energy= / normal= / count=, all True by default; one switched off is neither computed nor returned."""
    unknown = set(which) - set(POTENTIALS)
    if unknown:
        raise ValueError(f"unknown potential(s) {sorted(unknown)}")
    world.wait_download()
    world.sync_to_device(apply_removal=False)
    p = (params or Diffuse())._struct()
    mask, nrows = world._field_mask(fluids), C.c_uint64(0)
    L.check(world._L.salva_hip_diffuse_potentials(world._h, mask, C.byref(p), 0, None, C.byref(nrows)))
    n = int(nrows.value)
    got, out, _room = L.host_out(L.DiffusePotentialsOut, {k: (n, 3) if w == 3 else (n,) for k, w in POTENTIALS.items() if which.get(k, True)})
    out.row_capacity = n
    L.check(world._L.salva_hip_diffuse_potentials(world._h, mask, C.byref(p), 0, C.byref(out), C.byref(nrows)))
    return got


def potentials_device(world, params=None, fluids=None, row_capacity=0, **addresses):
    """LiquidWorld.diffuse_potentials_device: the keyword arguments are integer device addresses of buffers with room for
    `row_capacity` rows; one left out or 0 is not written.  Without any the call only counts.  Returns the number of rows."""
    unknown = set(addresses) - set(POTENTIALS)
    if unknown:
        raise ValueError(f"unknown potential(s) {sorted(unknown)}")
    world.wait_download()
    world.sync_to_device(apply_removal=False)
    p = (params or Diffuse())._struct()
    nrows, out = C.c_uint64(0), None
    if any(addresses.values()):
        out = L.device_out(L.DiffusePotentialsOut, addresses)
        out.row_capacity = int(row_capacity)
    L.check(world._L.salva_hip_diffuse_potentials(world._h, world._field_mask(fluids), C.byref(p), L.DIFFUSE_OUT_ON_DEVICE,
                                                  C.byref(out) if out is not None else None, C.byref(nrows)))
    return int(nrows.value)


KINDS = ("spray", "foam", "bubble", "new")


class DiffuseSet:
    """A set of diffuse particles in device memory (salva_hip_create_diffuse; LiquidWorld.create_diffuse): positions, velocities,
    lifetimes, kinds and ids in the order of creation.  `params` (a Diffuse) is what update() uses unless it is given another."""

    def __init__(self, world, capacity, params=None):
        self._world, self.capacity, self.params = world, int(capacity), params or Diffuse()
        h = C.c_uint32(0)
        L.check(world._L.salva_hip_create_diffuse(world._h, self.capacity, C.byref(h)))
        self._set = h.value

    def add(self, positions, velocities, lifetimes=None):
        """appends particles (kind "new"): this is how a user seeds"""
        x = np.ascontiguousarray(positions, F32).reshape(-1, 3)
        v = np.ascontiguousarray(velocities, F32).reshape(-1, 3)
        if len(v) != len(x):
            raise ValueError("one velocity per position")
        life = None if lifetimes is None else np.ascontiguousarray(np.broadcast_to(np.asarray(lifetimes, F32), (len(x),)))
        fp = C.POINTER(C.c_float)
        L.check(self._world._L.salva_hip_add_diffuse(self._world._h, self._set, len(x), x.ctypes.data_as(fp), v.ctypes.data_as(fp),
                                                     life.ctypes.data_as(fp) if life is not None else None, 0))

    def add_device(self, n, positions, velocities, lifetimes=0):
        """add() from device memory: integer device addresses of 3n, 3n and n floats (lifetimes 0: the default)"""
        fp = C.POINTER(C.c_float)
        L.check(self._world._L.salva_hip_add_diffuse(self._world._h, self._set, int(n), C.cast(C.c_void_p(int(positions)), fp),
                                                     C.cast(C.c_void_p(int(velocities)), fp),
                                                     C.cast(C.c_void_p(int(lifetimes)), fp) if lifetimes else None, L.DIFFUSE_IN_ON_DEVICE))

    def update(self, dt, params=None, fluids=None):
        """advect and age, remove, emit (salva_hip_update_diffuse), after a step of the world with the same dt"""
        w = self._world
        w.wait_download()
        w.sync_to_device(apply_removal=False)
        p = (params or self.params)._struct()
        L.check(w._L.salva_hip_update_diffuse(w._h, self._set, w._field_mask(fluids), C.byref(p), float(dt)))

    def __len__(self):
        n = C.c_uint64(0)
        L.check(self._world._L.salva_hip_get_diffuse(self._world._h, self._set, 0, None, C.byref(n)))
        return int(n.value)

    def get(self):
        """a dict of numpy arrays: positions, velocities (N x 3), lifetime, kind, id (N)"""
        n = len(self)
        got, out, _room = L.host_out(L.DiffuseOut, {"positions": (n, 3), "velocities": (n, 3), "lifetime": (n,), "kind": (n,), "id": (n,)})
        out.row_capacity = n
        m = C.c_uint64(0)
        L.check(self._world._L.salva_hip_get_diffuse(self._world._h, self._set, 0, C.byref(out), C.byref(m)))
        return got

    def get_device(self, row_capacity, **addresses):
        """get() into device memory: positions= / velocities= / lifetime= / kind= / id= are integer device addresses; returns N"""
        out = L.device_out(L.DiffuseOut, addresses)
        out.row_capacity = int(row_capacity)
        m = C.c_uint64(0)
        L.check(self._world._L.salva_hip_get_diffuse(self._world._h, self._set, L.DIFFUSE_OUT_ON_DEVICE, C.byref(out), C.byref(m)))
        return int(m.value)

    def stats(self):
        """count, the counts per kind, and emitted / dissolved / killed / dropped by the last update and in total"""
        st = L.DiffuseStats()
        L.check(self._world._L.salva_hip_get_diffuse_stats(self._world._h, self._set, C.byref(st)))
        out = {"count": int(st.count), **{k: int(st.kinds[i]) for i, k in enumerate(KINDS)}}
        for k in ("emitted", "dissolved", "killed", "dropped"):
            out[k], out["total_" + k] = int(getattr(st, k)), int(getattr(st, "total_" + k))
        return out

    def clear(self):
        L.check(self._world._L.salva_hip_clear_diffuse(self._world._h, self._set))

    def destroy(self):
        L.check(self._world._L.salva_hip_destroy_diffuse(self._world._h, self._set))
