"""One built-in NonPressureForce evaluated by the numpy reading (tests/numpy_reading.py) from a SNAPSHOT of the state the force saw,
instead of from a world the reading stepped itself: what a probe in front of and behind the force recorded — in the CPU oracle
(OracleWorld.add_custom_force) or on the device (a DeviceForce reader, include/salva_hip.h SalvaHipDeviceView) — goes in, the
force's own accelerations and its own boundary reactions come out.  tests/test_force_reading_cpu.py checks this harness against
the oracle's f64 build; tests/test_forces_isolated_gpu.py holds every force kernel to it.

Test infrastructure only."""
import numpy as np

from numpy_reading import DenseWorld, pair_tables


class Snapshot:
    """Everything a force reads, float64, particles of ALL fluids in one set of arrays (any order) and the particles of all
    boundaries in another:

      x, v (n, 3), m, rho (n), model (n: the fluid of each particle), rho0 (per fluid), acc (n, 3: the accelerations accumulated
      before the force — DFSPHViscosity reads them), xb, vb (nb, 3), volb (nb), bslot (nb: the boundary of each particle),
      h, kernels = (KernelDensity, KernelGradient) by name, dt / inv_dt as the timestep holds them at that point (the previous
      step's)."""

    def __init__(self, x, v, m, rho, model, rho0, acc, xb, vb, volb, bslot, h, kernels, dt, inv_dt):
        f8 = lambda a, shape: np.ascontiguousarray(np.asarray(a, np.float64).reshape(shape))
        self.x, self.v, self.acc = f8(x, (-1, 3)), f8(v, (-1, 3)), f8(acc, (-1, 3))
        self.m, self.rho, self.rho0 = f8(m, -1), f8(rho, -1), f8(rho0, -1)
        self.model = np.asarray(model, np.int64).reshape(-1)
        self.xb, self.vb, self.volb = f8(xb, (-1, 3)), f8(vb, (-1, 3)), f8(volb, -1)
        self.bslot = np.asarray(bslot, np.int64).reshape(-1)
        self.h, self.kernels, self.dt, self.inv_dt = float(h), tuple(kernels), float(dt), float(inv_dt)
        n, nb = len(self.x), len(self.xb)
        assert self.v.shape == self.acc.shape == (n, 3) and len(self.m) == len(self.rho) == len(self.model) == n
        assert self.vb.shape == (nb, 3) and len(self.volb) == len(self.bslot) == nb


class Reading:
    """A DenseWorld holding a Snapshot, its pair tables built once.  `f32_contacts`: the contact criterion in f32 arithmetic
    (pair_tables) — for snapshots of an f32 implementation, whose lists were decided that way; False for the oracle's f64 build.
    Everything else is f64.  No interaction group is filtered: the scenes that use this give every object the default groups."""

    def __init__(self, s, f32_contacts=True):
        w = DenseWorld(s.h / 4.0, 2.0, "dfsph", *s.kernels, f32_contacts=f32_contacts)
        assert w.h == s.h
        n, nb = len(s.x), len(s.xb)
        w.x, w.v, w.a, w.rho, w.model = s.x, s.v, s.acc.copy(), s.rho, s.model
        w.rho0 = s.rho0[s.model]
        w.vol = s.m / w.rho0
        w.nfluids = len(s.rho0)
        w.xb, w.vb, w.volb, w.bmodel = s.xb, s.vb, s.volb, s.bslot
        w.bforce = np.zeros((nb, 3))
        w.nboundaries = int(s.bslot.max()) + 1 if nb else 0
        w.dt, w.inv_dt = s.dt, s.inv_dt
        self.w, self.s = w, s
        self.m = s.m
        self.mb = s.volb[None, :] * w.rho0[:, None]   # V_b * fluid_i.density0
        self.full = (pair_tables(s.x, s.x, s.h, *s.kernels, f32_contacts=f32_contacts)
                     + pair_tables(s.x, s.xb, s.h, *s.kernels, f32_contacts=f32_contacts))

    # the contact lists' row lengths (self contacts and the other fluids' particles included, as the lists hold them)
    def ff_counts(self):
        return self.full[0].sum(axis=1)

    def fb_counts(self):
        return self.full[3].sum(axis=1)

    def force(self, fluid, force):
        """(accelerations (n, 3), boundary reaction (nb, 3)) of `force` = (kind, params...) in DenseWorld.add_force's terms, or
        ("xsph", fluid coefficient, boundary coefficient), sitting on `fluid`.  Rows of other fluids are zero.  The parameters are
        rounded to f32 first: that is how they cross the C ABI of the oracle and of the device library."""
        w = self.w
        w._mask_to_fluid(fluid, self.full)
        w.a = self.s.acc.copy()
        w.bforce = np.zeros_like(w.bforce)
        acc = getattr(w, "_force_" + force[0])(self.m, self.mb, *[float(np.float32(p)) for p in force[1:]])
        acc = np.where(w._rows[:, None], acc, 0.0)
        return acc, w.bforce.copy()

    # ---- what the terms of a force amount to on these inputs (tests/test_force_reading_cpu.py: the conditions on the inputs)
    def akinci_curvature(self, fluid, tension):
        """The curvature part of Akinci2013's fluid arm alone: sum_j k_ij (-tension) (n_i - n_j)."""
        w = self.w
        w._mask_to_fluid(fluid, self.full)
        normals = (w.gff * (self.m / w.rho)[None, :, None]).sum(axis=1) * w.h
        kij = 2.0 * w._rho0f / (w.rho[:, None] + w.rho[None, :])
        return ((normals[:, None, :] - normals[None, :, :]) * (-tension) * np.where(w.ff, kij, 0.0)[:, :, None]).sum(axis=1)

    def approaching(self, fluid):
        """(v_ij . r_ij < 0, v_ij . r_ij > 0) as boolean tables over the fluid's own fluid contacts (self contacts are neither) and
        over its boundary contacts."""
        w = self.w
        w._mask_to_fluid(fluid, self.full)
        out = []
        for mask, ox, ov in ((w.ff, w.x, w.v), (w.fb, w.xb, w.vb)):
            vr = ((w.x[:, None, :] - ox[None, :, :]) * (w.v[:, None, :] - ov[None, :, :])).sum(axis=2)
            out.append((mask & (vr < 0.0), mask & (vr > 0.0)))
        return out


def force_reading(snapshot, fluid, force, f32_contacts=True):
    return Reading(snapshot, f32_contacts).force(fluid, force)
