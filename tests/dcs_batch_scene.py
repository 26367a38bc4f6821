"""The scene of tests/test_dcs_batch_gpu.py: a 14^3 block of fluid (2 744 particles, R = 0.025) with six dynamically sampled
colliders in slot order — ball, cuboid, capsule, [a plain static boundary], cylinder, an oriented closed mesh (the unit cube of
mesh_fixtures, scaled and turned) and a height field — placed so that the loosened boxes of ball / cuboid and of capsule / cylinder
overlap INSIDE the fluid: particles in the overlap are pushed by the first collider of the pair and then, from where that push left
them, by the second.  The bodies are kinematic and move between the steps; the cylinder leaves for good after the second step, so
that one collider emits nothing in the third.

`analytic_prefix_pushes` restates the vacuity conditions of the test on the CPU oracle (which has no meshes: the five analytic
colliders, the mesh as the cuboid it is): rows emitted per collider, and how many particles two different colliders move in one step.
"""
import numpy as np

import mesh_fixtures as X
from parity import DT
from salva_amd import Boundary, DFSPHSolver, Fluid, LiquidWorld, NonPressureForce, XSPHViscosity, _lib, sampling, scenes
from salva_amd.coupling import ColliderCouplingSet, DynamicContactSampling, RigidBody

F = np.float32
R = 0.025
N = 14
MESH_HE = (0.10, 0.08, 0.12)
KIND = {"ball": 1, "cuboid": 2, "capsule": 3, "cylinder": 4}


class Probe(NonPressureForce):
    """Adds nothing; records the positions the solver works on: the state right after update_boundaries pushed particles out."""

    def __init__(self):
        self.positions = None

    def solve(self, timestep, kernel_radius, ff, fb, fluid, boundaries, densities):
        self.positions = fluid.positions.copy()


def fluid():
    pos = scenes.jitter(scenes.cube_fluid_positions(N, N, N, R), 0.2 * R, seed=15)
    pos[:, 1] += F(N * R)  # y in [0, 0.7]
    vel = scenes.random_velocities(len(pos), 0.6, seed=16)
    return pos, vel


def static_points():
    """A plain boundary: a 12 x 12 sheet next to the block's +x face (not sampled, not coupled; its rows must survive every relayout)."""
    g = (np.arange(12, dtype=F) * F(2 * R)) + F(0.05)
    y, z = np.meshgrid(g, g - F(0.3), indexing="ij")
    return np.stack([np.full(y.size, F(0.40)), y.ravel(), z.ravel()], axis=1).astype(F)


def _body(t, axis=(0.0, 0.0, 0.0), linvel=(0.0, 0.0, 0.0), angvel=(0.0, 0.0, 0.0), com=(0.0, 0.0, 0.0)):
    return RigidBody(translation=F(t), rotation=scenes.quat_from_scaled_axis(axis) if any(axis) else F([0, 0, 0, 1]), linvel=F(linvel),
                     angvel=F(angvel), local_com=F(com), dynamic=False)


def mesh_cuboid():
    v, t, _ = X.cube()
    return (v * (F(2) * F(MESH_HE))).astype(F), t, True


def heightfield():
    v, t, _ = X.heightfield9()
    return (v * F([0.8, 0.04, 0.8])).astype(F), t, False


def colliders():
    """[(name, shape, body)] in slot order (the static boundary goes between "capsule" and "cylinder"); fresh bodies every call."""
    return [
        ("ball", ("ball", 0.13), _body([-0.15, 0.30, -0.10], linvel=[0.4, 0.3, -0.2], angvel=[1.0, -2.0, 0.5], com=[0.01, 0.0, -0.02])),
        ("cuboid", ("cuboid", (0.12, 0.10, 0.14)), _body([-0.05, 0.34, -0.04], axis=(0.3, -0.2, 0.5), linvel=[-0.3, 0.2, 0.1], angvel=[-0.5, 1.0, 2.0])),
        ("capsule", ("capsule", 0.08, 0.07), _body([0.17, 0.22, 0.14], axis=(0.4, 0.1, -0.3), linvel=[0.1, -0.2, 0.3], angvel=[0.5, 0.5, -1.0])),
        ("cylinder", ("cylinder", 0.06, 0.10), _body([0.14, 0.27, 0.10], axis=(-0.2, 0.3, 0.6), linvel=[-0.2, 0.4, 0.0], angvel=[2.0, 0.0, 1.0])),
        ("mesh", "mesh", _body([0.02, 0.58, 0.12], axis=(0.2, 0.4, -0.1), linvel=[0.0, -0.5, 0.2], angvel=[0.0, 1.5, 0.5])),
        ("heightfield", "heightfield", _body([0.0, -0.06, 0.0], linvel=[0.0, 0.5, 0.0])),
    ]


def move(bodies, step):
    """Between the steps: every body goes on along its velocities; the cylinder leaves after the second step."""
    for name, _, body in bodies:
        body.integrate(DT, (0.0, 0.0, 0.0))
        if name == "cylinder" and step == 1:
            body.translation = (body.translation + F([40.0, 0.0, 0.0])).astype(F)


def sampling_of(shape):
    if shape == "mesh":
        v, t, oriented = mesh_cuboid()
        return DynamicContactSampling(sampling.Mesh(v, t, oriented=oriented))
    if shape == "heightfield":
        v, t, oriented = heightfield()
        return DynamicContactSampling(sampling.Mesh(v, t, oriented=oriented))
    return DynamicContactSampling(shape)


def hip_world(pos, vel, cols, static_after=2, probe=None, solver=None, set_dt=True):
    """-> world, fluid handle, [boundary per collider], static boundary (None: static_after < 0), coupling set"""
    w = LiquidWorld(solver or DFSPHSolver(), R, 2.0)
    fl = Fluid(pos, R, 1000.0)
    fl.velocities = vel
    fl.nonpressure_forces.append(XSPHViscosity(0.5, 0.5))
    if probe is not None:
        fl.nonpressure_forces.append(probe)
    h = w.add_fluid(fl)
    bounds, static, c = [], None, ColliderCouplingSet()
    for k, (name, shape, body) in enumerate(cols):
        b = w.add_boundary(Boundary(np.zeros((0, 3), F)))
        c.register_coupling(b, name, body, shape if not isinstance(shape, (tuple, str)) else sampling_of(shape))
        bounds.append(b)
        if k == static_after:
            static = w.add_boundary(Boundary(static_points()))
    w.sync_to_device()
    if set_dt:  # a previous substep length, as a continued run carries it: the prediction x + v dt is exercised from the first step
        _lib.check(w._L.salva_hip_set_timestep(w._h, DT, 1.0 / DT))
    return w, h, bounds, static, c


def dcs_stats(w):
    import ctypes as C

    out = (C.c_uint64 * 4)()
    _lib.check(w._L.salva_hip_get_dcs_stats(w._h, out))
    return [int(x) for x in out]  # passes over the fluid, host waits, batched colliders, records


def oracle_world(pos, vel, cols, probe=None):
    """The analytic colliders of `cols` (the mesh as the cuboid it is; the height field left out) in the CPU oracle."""
    from oracle import oracle as O

    o = O.OracleWorld(R, 2.0, O.DFSPH)
    f = o.add_fluid(pos, 1000.0, vel)
    o.add_xsph(f, 0.5, 0.5)
    if probe is not None:
        o.add_custom_force(f, lambda world, fl, positions, velocities, densities, acc: probe.append(positions.astype(F)))
    k = 0
    for name, shape, body in cols:
        if shape == "heightfield":
            continue
        if shape == "mesh":
            shape = ("cuboid", MESH_HE)
        b = o.add_boundary(np.zeros((0, 3), F))
        params = [float(x) for x in (shape[1] if shape[0] == "cuboid" else shape[1:])]
        o.set_boundary_dynamic_sampling(b, KIND[shape[0]], params)
        o.update_boundary_pose(k, body.translation, body.rotation, body.linvel, body.angvel, body.center_of_mass(), True, False)
        k += 1
    o.set_timestep(DT, 1.0 / DT)
    return o, f


def analytic_prefix_pushes(pos, vel, cols):
    """One oracle step per prefix of the analytic colliders: collider k moved particle i iff the pushed positions of prefix k differ
    from those of prefix k - 1 there.  -> rows emitted per collider (all colliders), movers per particle"""
    cols = [c for c in cols if c[1] != "heightfield"]
    movers = np.zeros(len(pos), int)
    prev = pos
    for k in range(1, len(cols) + 1):
        probe = []
        o, _ = oracle_world(pos, vel, cols[:k], probe)
        o.step(DT, (0.0, -9.81, 0.0))
        movers += (np.abs(probe[0] - prev).max(axis=1) > 0)
        prev = probe[0]
        if k == len(cols):
            rows = [o.boundary_len(b) for b in range(k)]
    return rows, movers
