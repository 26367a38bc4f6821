"""Re-registering a boundary slot releases what the slot held and behaves like a fresh registration (world.h DynSampling,
world_coupling.hip).  A slot is a plain upload, statically sampled, or dynamically sampled by a ball, a host shape, a mesh or a
compound; for every ordered pair (A -> B): slot 1 is registered as A, the world steps, the slot is registered as B through the C entry
points, the world steps again.  Then

  - every mesh and compound handle only A used can be destroyed, which the library refused while A was registered;
  - the slot's rows equal, bit for bit, those of a world that never knew A: the first world's fluid after its first step, uploaded,
    slot 1 registered as B from the start.  The two worlds hold their particles in different orders (one has sorted them once), and
    the emission of a dynamically sampled boundary follows that order, so its rows are compared by source particle: each fluid
    particle emits at most one row per collider;
  - a host shape's callbacks are not called once the slot is something else, after salva_hip_clear_boundary_sampling as well.

The fluid block and the collider poses are those of tests/dcs_batch_scene.py; a plain boundary sits in the slot before and in the slot
behind, whose rows move whenever slot 1 changes its length."""
import ctypes as C

import numpy as np
import pytest

import dcs_batch_scene as S
from parity import DT, GRAVITY
from salva_amd import Boundary, DFSPHSolver, Fluid, LiquidWorld, _lib, sampling
from salva_amd.coupling import HostShapeSampling, make_shape
from test_host_shape_gpu import cuboid_callbacks

pytestmark = pytest.mark.gpu

F = np.float32
FP = C.POINTER(C.c_float)
KINDS = ["plain", "static", "ball", "host", "mesh", "compound"]
DYNAMIC = ("ball", "host", "mesh", "compound")
BEHIND = (S.static_points() + F([0.05, 0.0, 0.0])).astype(F)
_FLUID = []


def _fluid():
    if not _FLUID:
        _FLUID.extend(S.fluid())
    return _FLUID


def _fp(a):
    return a.ctypes.data_as(FP)


def _world(pos, vel):
    """-> world, fluid, the boundary of slot 1 (empty, left to the C entry points from here on), the plain boundary behind it"""
    w = LiquidWorld(DFSPHSolver(), S.R, 2.0)
    fl = Fluid(pos, S.R, 1000.0)
    fl.velocities = vel
    h = w.add_fluid(fl)
    w.add_boundary(Boundary(S.static_points()))
    slot = w.add_boundary(Boundary(np.zeros((0, 3), F)))
    behind = w.add_boundary(Boundary(BEHIND))
    w.sync_to_device()
    slot._sampled = True  # (the Python world never uploads it again)
    assert slot._slot == 1
    _lib.check(w._L.salva_hip_set_timestep(w._h, DT, 1.0 / DT))
    return w, h, slot, behind


class Registration:
    """Slot 1 of `w` as `kind`, and what only this registration uses."""

    def __init__(self, w, kind):
        L, h = w._L, w._h
        bodies = {name: body for name, _, body in S.colliders()}
        self.kind, self.meshes, self.compound, self.calls, self.host = kind, [], None, [0, 0], None
        body = None
        if kind == "plain":
            self.points = (S.static_points() + F([-0.85, 0.0, 0.0])).astype(F)
            _lib.check(L.salva_hip_set_boundary(h, 1, len(self.points), _fp(self.points), _fp(np.zeros_like(self.points)), 1, 0xffffffff, 0))
        elif kind == "static":
            local = (S.static_points() - F([0.40, 0.30, 0.0])).astype(F)
            _lib.check(L.salva_hip_set_boundary_sampling(h, 1, len(local), _fp(local), 1, 0xffffffff))
            body = bodies["ball"]
        elif kind == "ball":
            _lib.check(L.salva_hip_set_boundary_dynamic_sampling(h, 1, C.byref(make_shape(("ball", 0.13))), 1, 0xffffffff))
            body = bodies["ball"]
        elif kind == "host":
            body = bodies["cuboid"]
            aabb, project = cuboid_callbacks(body, (0.12, 0.10, 0.14))

            def counted(k, f):
                def g(*a):
                    self.calls[k] += 1
                    return f(*a)
                return g

            self.host = HostShapeSampling(counted(0, aabb), counted(1, project))  # (keeps the ctypes thunks alive)
            _lib.check(L.salva_hip_set_boundary_dynamic_sampling_host(h, 1, C.byref(self.host.shape), 1, 0xffffffff))
        elif kind == "mesh":
            self.meshes = [sampling.Mesh(*S.mesh_cuboid())]
            _lib.check(L.salva_hip_set_boundary_dynamic_sampling_mesh(h, 1, self.meshes[0].handle(w), 1, 0xffffffff))
            body = bodies["mesh"]
        else:
            v, t, oriented = S.mesh_cuboid()
            self.meshes = [sampling.Mesh((v * F(0.5)).astype(F), t, oriented)]
            self.compound = sampling.Compound([(("ball", 0.07), (0.06, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)),
                                               (("cuboid", (0.05, 0.06, 0.04)), (-0.06, 0.02, 0.0), (0.0, 0.0, 0.0, 1.0)),
                                               (self.meshes[0], (0.0, -0.05, 0.05), (0.0, 0.0, 0.0, 1.0))])
            _lib.check(L.salva_hip_set_boundary_dynamic_sampling_compound(h, 1, self.compound.handle(w), 1, 0xffffffff))
            body = bodies["capsule"]
        if body is not None:
            _lib.check(L.salva_hip_update_boundary_pose(h, 1, C.byref(body.pose())))

    def destroy_handles(self, w):
        """The compound, then its and the registration's meshes (a compound keeps its meshes)."""
        if self.compound is not None:
            self.compound.destroy(w)
        for m in self.meshes:
            m.destroy(w)

    def handles_refused(self, w):
        held = ([self.compound] if self.compound is not None else []) + self.meshes  # (a mesh part is held by its compound)
        for x in held:
            with pytest.raises(_lib.SalvaHipError):
                x.destroy(w)
        return len(held)


def _rows(w, slot, dynamic):
    """The slot's rows; those of a dynamically sampled boundary in the order of their source particles."""
    pos, vel = (np.array(a, F).reshape(-1, 3) for a in w._boundary_particles(slot))
    if not dynamic:
        return pos, vel, None
    fs, idx = slot.sources()
    assert not fs.any() and len(np.unique(idx)) == len(idx)
    order = np.argsort(idx, kind="stable")
    return pos[order], vel[order], idx[order]


@pytest.mark.parametrize("b_kind", KINDS)
@pytest.mark.parametrize("a_kind", KINDS)
def test_reregistering_a_slot_releases_and_starts_afresh(a_kind, b_kind):
    pos, vel = _fluid()
    w, h, slot, behind = _world(pos, vel)
    slot._dynamic = True  # (num_particles: the device knows the count)
    a = Registration(w, a_kind)
    w.step(DT, GRAVITY)
    if a_kind in DYNAMIC:
        assert slot.num_particles() > 0, "A emits nothing: the slot has nothing to release"
    refused = a.handles_refused(w)
    assert refused == {"mesh": 1, "compound": 2}.get(a_kind, 0)
    mid_pos, mid_vel = np.array(h.positions, F), np.array(h.velocities, F)
    calls_a = list(a.calls)
    if a_kind == "host":
        assert min(calls_a) >= 1
    b = Registration(w, b_kind)
    w.step(DT, GRAVITY)
    # ---- what only A used is free again, and A's callbacks are not called any more
    a.destroy_handles(w)
    assert a.calls == calls_a, "a host callback of the replaced registration was called"
    # ---- the slot is what a world that never knew A holds
    w2, h2, slot2, behind2 = _world(mid_pos, mid_vel)
    slot2._dynamic = True
    b2 = Registration(w2, b_kind)
    w2.step(DT, GRAVITY)
    got, want = _rows(w, slot, b_kind in DYNAMIC), _rows(w2, slot2, b_kind in DYNAMIC)
    print(a_kind, "->", b_kind, "rows", len(got[0]), "fresh world", len(want[0]), "host calls", a.calls, b.calls, b2.calls)
    if b_kind in DYNAMIC:
        assert len(want[0]) >= 1, "B emits nothing: the comparison is of empty arrays"
    for x, y, what in zip(got, want, ("positions", "velocities", "source particles")):
        assert (x is None and y is None) or np.array_equal(x, y), f"{a_kind} -> {b_kind}: the slot's {what} differ from a fresh registration's"
    # the plain boundary behind the slot moved with every change of length and is intact
    for world, bd in ((w, behind), (w2, behind2)):
        p, v = world._boundary_particles(bd)
        assert np.array_equal(np.array(p, F), BEHIND) and not np.array(v).any()


@pytest.mark.parametrize("how", ["clear", "plain"])
def test_no_host_callback_after_the_slot_stopped_being_a_host_shape(how):
    pos, vel = _fluid()
    w, h, slot, behind = _world(pos, vel)
    slot._dynamic = True
    a = Registration(w, "host")
    w.step(DT, GRAVITY)
    assert min(a.calls) >= 1 and slot.num_particles() > 0
    calls = list(a.calls)
    if how == "clear":
        _lib.check(w._L.salva_hip_clear_boundary_sampling(w._h, 1))
    else:
        Registration(w, "plain")
    w.step(DT, GRAVITY)
    w.step(DT, GRAVITY)
    assert a.calls == calls
