"""Compound colliders on the device (salva_hip_create_compound; compound.h) in their three consumers — the per-collider
arm of DynamicContactSampling (k_dcs_compound_project), the batched arm (k_dcsb_segment) and the shape queries (k_compound_query,
k_mesh_query) — against the numpy reading of tests/compound_reading.py, bit for bit where both sides are f32 restatements of each
other.  The fluid of (a), (d) and (e) is test_host_shape_gpu._scene(): 14^3 particles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import compound_reading as CR
import compound_scenes as CS
import dcs_batch_scene as S
from parity import DT, GRAVITY
from salva_amd import Boundary, DFSPHSolver, Fluid, LiquidWorld, NonPressureForce, XSPHViscosity, _lib, dist, sampling, scenes
from salva_amd.coupling import ColliderCouplingSet, DynamicContactSampling, FluidsPipeline, HostShapeSampling, RigidBody
from test_dcs_batch_gpu import _run_pair
from test_host_shape_gpu import R as RAD, _scene, cuboid_callbacks
from test_mesh_dcs_gpu import _compare

pytestmark = pytest.mark.gpu

F = np.float32
FP = C.POINTER(C.c_float)
U32P = C.POINTER(C.c_uint32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 256  # common.h
ZERO_G = (0.0, 0.0, 0.0)


def last_error(w):
    return w._L.salva_hip_last_error().decode()


def _world(pos, vel, colliders, host, probe=None):
    """colliders: [(body, parts or a shape tuple, log)]; host: HostShapeSampling over the reading instead of the device arm."""
    w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    fl = Fluid(pos, RAD, 1000.0)
    fl.velocities = vel
    fl.nonpressure_forces.append(XSPHViscosity(0.5, 0.5))
    if probe is not None:
        fl.nonpressure_forces.append(probe)
    h = w.add_fluid(fl)
    bounds = [w.add_boundary(Boundary(np.zeros((0, 3), F))) for _ in colliders]
    c = ColliderCouplingSet()
    for k, (body, parts, log) in enumerate(colliders):
        if isinstance(parts, tuple):
            method = DynamicContactSampling(parts)
        elif host:
            method = HostShapeSampling(*CR.callbacks(parts, body, log))
        else:
            method = DynamicContactSampling(CR.to_compound(parts))
        c.register_coupling(bounds[k], k, body, method)
    w.sync_to_device()
    _lib.check(w._L.salva_hip_set_timestep(w._h, DT, 1.0 / DT))  # (so that the prediction x + v dt is exercised from the first step)
    return w, h, bounds, c


# ---------------------------------------------------------------------------------------------- (a) against the host arm
def test_compounds_match_the_host_arm_bit_for_bit():
    """A cuboid, a capsule and an oriented tetrahedron that overlap, on the moving and spinning body; two slabs and a cylinder on the
    tilted one.  On the CPU beforehand (the reading on the first step's predictions): 549 and 788 points emit, 25 and 35 lie inside,
    and every part of both compounds wins for more than 100 of them."""
    pos, vel, slab_a, body_a = _scene()
    _, _, slab_b, body_b = _scene()
    pushed = [[], []]
    wa, ha, ba, ca = _world(pos, vel, [(slab_a, CS.slab_compound(), None), (body_a, CS.body_compound(), None)], host=False)
    wb, hb, bb, cb = _world(pos, vel, [(slab_b, CS.slab_compound(), pushed[0]), (body_b, CS.body_compound(), pushed[1])], host=True)
    most = [0, 0]
    for step in range(6):
        wa.step_with_coupling(DT, GRAVITY, ca)
        wb.step_with_coupling(DT, GRAVITY, cb)
        for body in (body_a, body_b):
            body.integrate(DT, (0.0, 0.0, 0.0))
        counts = _compare(step, ha, hb, ba, bb)
        most = [max(m, c) for m, c in zip(most, counts)]
    print("emitted (max per boundary)", most, "particles inside per step", pushed)
    assert most[0] > 50 and most[1] > 50
    assert max(pushed[0] + pushed[1]) >= 1, "no particle was ever inside a compound: the push-out branch was not covered"


# ---------------------------------------------------------------------------------------------- (b) the projection on fixed clouds
def _cloud_case(parts, body, pts):
    """One step of a world whose fluid is `pts` at rest -> the compound's rows against the reading's projection of every point, and
    the pushed positions against the reading's push-out."""
    probe = S.Probe()
    w, h, (b,), c = _world(pts, np.zeros_like(pts), [(body, parts, None)], host=False, probe=probe)
    w.step_with_coupling(DT, ZERO_G, c)
    winners = []
    proj, inside = CR.project(parts, body, pts, winners)
    keep = CS.emits(pts, proj, inside)
    fs, src = b.sources()
    order = np.argsort(src, kind="stable")
    assert np.array_equal(src[order], np.nonzero(keep)[0]), "different points emitted"
    assert np.array_equal(np.array(b.positions, F)[order], proj[keep]), "projections differ"
    # the push-out of the points inside (dcs.hip dcs_finish_reg), f32
    d = (pts - proj).astype(F)
    sq = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.sqrt(sq)
        n = (d / depth[:, None]).astype(F)
        m = (depth + F(F(RAD) * F(0.1))).astype(F)
        out = (pts - (n * m[:, None]).astype(F)).astype(F)
    moved = inside & (sq > CS.EPS * CS.EPS)
    want = np.where(moved[:, None], out, pts)
    assert np.array_equal(probe.positions, want), "pushed positions differ"
    return winners[0], inside, keep


@pytest.mark.parametrize("count", [1, 63, 64, 65, BLOCK + 1])
def test_projection_on_fixed_clouds(count):
    parts = CS.body_compound()
    body = RigidBody(translation=F([0.02, 0.03, -0.01]), rotation=CS.quat((0.3, -0.2, 0.5)), linvel=F([0.2, -0.1, 0.3]), angvel=F([1.0, 2.0, -0.5]),
                     dynamic=False)
    who, inside, keep = _cloud_case(parts, body, CS.lattice_cloud(body.translation, count))
    print(count, "points; winners per part", np.bincount(who[who >= 0], minlength=3), "inside", int(inside.sum()), "emitting", int(keep.sum()))
    if count > 64:  # points on both sides of every part, every part wins somewhere
        assert inside.any() and not inside.all() and (np.bincount(who[who >= 0], minlength=3) > 0).all()
        for part in parts:
            ins = CR.part_project(part, CR.to_local(body, CS.lattice_cloud(body.translation, count)))[1]
            assert ins.any() and not ins.all()


def test_projection_tie_and_nearer_part():
    body = RigidBody(dynamic=False)  # (identity: the local coordinates are exact)
    parts, points = CS.mirrored_balls()
    who, _, keep = _cloud_case(parts, body, points)
    assert (who == 0).all() and keep.all()
    parts, point = CS.deep_in_a_near_b()
    who, inside, keep = _cloud_case(parts, body, point)
    assert who[0] == 1 and not inside[0] and keep[0]


def test_projection_with_parts_far_apart():
    parts = CS.far_apart()
    body = RigidBody(translation=F([0.0, 0.0, 0.0]), rotation=CS.quat((0.1, 0.2, -0.1)), dynamic=False)
    pts = np.concatenate([CS.lattice_cloud(CR.to_world(body, np.asarray(t, F)[None])[0], 40, seed=30 + k) for k, (_, t, _) in enumerate(parts)])
    who, inside, keep = _cloud_case(parts, body, pts)
    assert (np.bincount(who, minlength=5) >= 20).all() and inside.any() and keep.sum() > 100


# ---------------------------------------------------------------------------------------------- (c) batching
def _small_compound():
    return [(("ball", 0.06), F([0.0, 0.03, 0.0]), CS.ID), (("cuboid", (0.07, 0.03, 0.05)), F([0.02, -0.03, 0.0]), CS.quat((0.0, 0.4, 0.2)))]


def _batch_cols(host_between=False):
    """ball, compound, mesh, compound on the bodies of the batch scene's first colliders (all inside the block, loosened boxes
    overlapping); host_between: a host-shape cuboid after the first compound."""
    base = {n: b for n, _, b in S.colliders()}
    cols = [("ball", ("ball", 0.13), base["ball"]),
            ("compound0", DynamicContactSampling(CR.to_compound(CS.body_compound())), base["cuboid"])]
    if host_between:
        body = RigidBody(translation=F([0.06, 0.34, 0.04]), rotation=CS.quat((0.3, -0.2, 0.5)), linvel=F([-0.3, 0.2, 0.1]), dynamic=False)
        cols.append(("host", HostShapeSampling(*cuboid_callbacks(body, (0.12, 0.10, 0.14))), body))
    mesh_body = base["mesh"]
    mesh_body.translation = F([0.02, 0.45, 0.12])
    cols += [("mesh", "mesh", mesh_body), ("compound1", DynamicContactSampling(CR.to_compound(_small_compound())), base["capsule"])]
    return cols


def test_batched_run_with_compounds_equals_the_per_collider_path(monkeypatch):
    pos, vel = S.fluid()
    (sb, stats_b, _), (sp, stats_p, _) = _run_pair(monkeypatch, pos, vel, _batch_cols, 3, static_after=1)
    rows = [[s[f"b{k}_n"] for k in range(4)] for s in sp]
    print("rows per collider and step:", rows, "stats batched", stats_b, "per collider", stats_p)
    assert min(rows[0]) > 20, rows[0]
    assert np.abs(sp[0]["pushed"] - pos).max() > 0
    assert all(s[2] == 4 for s in stats_b) and all(s[2] == 0 for s in stats_p)
    assert all(s[0] == 1 and s[1] == 1 for s in stats_b[1:]), stats_b  # (the first step may repeat its pass to size the record buffer)
    assert all(s[0] == 4 for s in stats_p)


def test_a_host_shape_splits_a_run_with_compounds(monkeypatch):
    pos, vel = S.fluid()
    (sb, stats_b, _), (sp, stats_p, _) = _run_pair(monkeypatch, pos, vel, lambda: _batch_cols(True), 2, static_after=-1)
    assert all(sp[0][f"b{k}_n"] > 20 for k in range(5)), [sp[0][f"b{k}_n"] for k in range(5)]
    for s in stats_b[1:]:
        assert s[2] == 4 and s[0] == 3, s   # two batches of two around the host arm
    for s in stats_p:
        assert s[2] == 0 and s[0] == 5, s


def test_record_buffer_growth_with_compounds(monkeypatch):
    pos, vel = S.fluid()
    (sb, stats_b, _), _ = _run_pair(monkeypatch, pos, vel, _batch_cols, 2, env={"SALVA_HIP_DCSB_CAP0": "1"}, static_after=-1)
    assert stats_b[0][0] >= 2 and stats_b[0][2] == 4, stats_b  # the first pass did not fit and was repeated from the unmodified state
    assert stats_b[1][0] == 1 and stats_b[1][1] == 1, stats_b


# ---------------------------------------------------------------------------------------------- (d) a one-part compound
def test_a_one_part_compound_equals_the_plain_shape():
    from test_host_shape_gpu import BALL_R, CUBOID_HE

    pos, vel, slab_a, body_a = _scene()
    _, _, slab_b, body_b = _scene()
    one = lambda shape: [(shape, np.zeros(3, F), CS.ID)]  # noqa: E731
    wa, ha, ba, ca = _world(pos, vel, [(slab_a, one(("cuboid", CUBOID_HE)), None), (body_a, one(("capsule", 0.06, BALL_R)), None)], host=False)
    wb, hb, bb, cb = _world(pos, vel, [(slab_b, ("cuboid", CUBOID_HE), None), (body_b, ("capsule", 0.06, BALL_R), None)], host=False)
    for step in range(3):
        wa.step_with_coupling(DT, GRAVITY, ca)
        wb.step_with_coupling(DT, GRAVITY, cb)
        for body in (body_a, body_b):
            body.integrate(DT, (0.0, 0.0, 0.0))
        counts = _compare(step, ha, hb, ba, bb)
        assert min(counts) > 50 or step > 0, counts


# ---------------------------------------------------------------------------------------------- (e) queries
def _hits(found):
    return sorted((kind, id(owner), i) for kind, owner, i in found)


def test_queries_equal_the_host_shape_query():
    pos, _, _, _ = _scene()
    w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    w.add_fluid(Fluid(pos, RAD, 1000.0))
    w.add_boundary(Boundary(S.static_points() + F([-0.3, 0.1, 0.3])))
    w.sync_to_device()
    body = CR.pose([0.05, 0.33, -0.02], CS.quat((0.4, -0.3, 0.2)))
    parts = CS.body_compound()
    got = w.particles_intersecting_shape(body.translation, body.rotation, CR.to_compound(parts))
    want = w.particles_intersecting_host_shape(lambda: CR.aabb(parts, body), lambda p: CR.distance(parts, body, p))
    print("compound query:", len(got), "particles")
    assert len(got) > 100 and _hits(got) == _hits(want)
    assert {k for k, _, _ in got} == {"fluid", "boundary"}
    # an oriented cube mesh: against the reading's distance, and against the cuboid it is
    he = (0.12, 0.07, 0.16)
    cube = CS.cube_mesh(he)
    mesh = sampling.Mesh(cube[1], cube[2], oriented=True)
    got = w.particles_intersecting_shape(body.translation, body.rotation, mesh)
    one = [(cube, np.zeros(3, F), CS.ID)]
    want = w.particles_intersecting_host_shape(lambda: CR.aabb(one, body), lambda p: CR.distance(one, body, p))
    assert len(got) > 100 and _hits(got) == _hits(want)
    assert _hits(got) == _hits(w.particles_intersecting_shape(body.translation, body.rotation, ("cuboid", he)))
    # capacity: the total is reported, the first `capacity` hits are written
    t, q = (C.c_float * 3)(*body.translation), (C.c_float * 4)(*body.rotation)
    k, s, i = (np.zeros(8, np.uint32) for _ in range(3))
    n = w._L.salva_hip_particles_intersecting_mesh(w._h, t, q, mesh.handle(w), 8, k.ctypes.data_as(U32P), s.ctypes.data_as(U32P), i.ctypes.data_as(U32P))
    assert n == len(got)


# ---------------------------------------------------------------------------------------------- (f) errors and lifetimes
def _part(kind=_lib.SHAPE_BALL, params=(0.1, 0.1, 0.1), mesh=0, t=(0, 0, 0), q=(0, 0, 0, 1)):
    p = _lib.CompoundPart()
    p.kind, p.mesh = kind, mesh
    p.params[:] = params
    p.translation[:] = t
    p.rotation_ijkw[:] = q
    return p


def _create(w, parts, n=None):
    arr = (_lib.CompoundPart * max(len(parts), 1))(*parts)
    h = C.c_uint32(0xFFFFFFFF)
    return w._L.salva_hip_create_compound(w._h, arr, len(parts) if n is None else n, C.byref(h)), h.value


def test_errors_and_handle_lifetimes():
    w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    w.add_fluid(Fluid(scenes.cube_fluid_positions(4, 4, 4, RAD), RAD, 1000.0))
    b = w.add_boundary(Boundary(np.zeros((0, 3), F)))
    w.sync_to_device()
    L = w._L
    nan, inf = float("nan"), float("inf")
    assert _create(w, [], 0)[0] == _lib.E_INVALID
    assert _create(w, [_part()] * 65)[0] == _lib.E_INVALID
    assert _create(w, [_part()] * 64)[0] == _lib.OK
    for kind in (0, _lib.SHAPE_COMPOUND, 100, 7):  # nothing, nesting, a host part, unknown
        assert _create(w, [_part(), _part(kind=kind)])[0] == _lib.E_INVALID, kind
    for bad in (0.0, -0.1, nan, inf):
        assert _create(w, [_part(params=(bad, 0.1, 0.1))])[0] == _lib.E_INVALID, bad
        assert _create(w, [_part(kind=_lib.SHAPE_CUBOID, params=(0.1, 0.1, bad))])[0] == _lib.E_INVALID, bad
        assert _create(w, [_part(kind=_lib.SHAPE_CAPSULE, params=(0.1, bad, 0.0))])[0] == _lib.E_INVALID, bad
    assert _create(w, [_part(kind=_lib.SHAPE_CAPSULE, params=(0.1, 0.1, 0.0))])[0] == _lib.OK  # (the unused parameter is not looked at)
    assert _create(w, [_part(t=(0, nan, 0))])[0] == _lib.E_INVALID
    assert _create(w, [_part(t=(inf, 0, 0))])[0] == _lib.E_INVALID
    assert _create(w, [_part(q=(0, 0, 0, 1.01))])[0] == _lib.E_INVALID
    assert _create(w, [_part(q=(0, 0, 0, 1.0004))])[0] == _lib.OK
    assert _create(w, [_part(q=(0, nan, 0, 1))])[0] == _lib.E_INVALID
    assert _create(w, [_part(kind=_lib.SHAPE_MESH, mesh=12345)])[0] == _lib.E_INVALID and "no such mesh" in last_error(w)
    assert L.salva_hip_destroy_compound(w._h, 12345) == _lib.E_INVALID

    # a compound shares ownership of its meshes
    tet = CS.tetra()
    mesh = sampling.Mesh(tet[1], tet[2], oriented=True)
    def make():
        rc, handle = _create(w, [_part(), _part(kind=_lib.SHAPE_MESH, mesh=mesh.handle(w), t=(0.1, 0, 0))])
        assert rc == _lib.OK
        return handle

    def register(handle):
        return L.salva_hip_set_boundary_dynamic_sampling_compound(w._h, b._slot, handle, 1, 0xFFFFFFFF)

    first, second, third, fourth = make(), make(), make(), make()
    assert len({first, second, third, fourth}) == 4
    assert L.salva_hip_destroy_mesh(w._h, mesh.handle(w)) == _lib.E_INVALID and "compound" in last_error(w)

    # a dynamically sampled boundary keeps its compound; each of the three releases lets go of it, checked by a destroy right after
    assert register(12345) == _lib.E_INVALID
    # ... salva_hip_clear_boundary_sampling
    assert register(first) == _lib.OK
    w.step(DT, GRAVITY)
    assert L.salva_hip_destroy_compound(w._h, first) == _lib.E_INVALID and "salva_hip_clear_boundary_sampling" in last_error(w)
    assert L.salva_hip_clear_boundary_sampling(w._h, b._slot) == _lib.OK
    assert L.salva_hip_destroy_compound(w._h, first) == _lib.OK
    assert L.salva_hip_destroy_compound(w._h, first) == _lib.E_INVALID  # gone
    assert register(first) == _lib.E_INVALID
    # ... a re-registration of the slot: with a built-in shape, with another compound
    assert register(second) == _lib.OK
    assert L.salva_hip_destroy_compound(w._h, second) == _lib.E_INVALID
    ball = _lib.Shape()
    ball.kind, ball.params[0] = _lib.SHAPE_BALL, 0.1
    assert L.salva_hip_set_boundary_dynamic_sampling(w._h, b._slot, C.byref(ball), 1, 0xFFFFFFFF) == _lib.OK
    assert L.salva_hip_destroy_compound(w._h, second) == _lib.OK
    assert register(third) == _lib.OK
    assert register(fourth) == _lib.OK
    assert L.salva_hip_destroy_compound(w._h, third) == _lib.OK
    assert L.salva_hip_destroy_compound(w._h, fourth) == _lib.E_INVALID
    w.step(DT, GRAVITY)
    # ... the boundary's removal
    assert L.salva_hip_remove_boundary(w._h, b._slot) == _lib.OK
    assert L.salva_hip_destroy_mesh(w._h, mesh.handle(w)) == _lib.E_INVALID  # (the last compound still names the mesh)
    assert L.salva_hip_destroy_compound(w._h, fourth) == _lib.OK
    assert L.salva_hip_destroy_mesh(w._h, mesh.handle(w)) == _lib.OK    # ... and with it the hold on the mesh went

    # the queries need a solid distance
    w2 = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    w2.add_fluid(Fluid(scenes.cube_fluid_positions(4, 4, 4, RAD), RAD, 1000.0))
    w2.sync_to_device()
    surface = sampling.Mesh(tet[1], tet[2], oriented=False)
    t, q = (C.c_float * 3)(0, 0, 0), (C.c_float * 4)(0, 0, 0, 1)
    assert w2._L.salva_hip_particles_intersecting_mesh(w2._h, t, q, surface.handle(w2), 0, None, None, None) == _lib.E_INVALID
    assert "salva_hip_particles_intersecting_host_shape" in last_error(w2)
    rc, comp = _create(w2, [_part(), _part(kind=_lib.SHAPE_MESH, mesh=surface.handle(w2))])
    assert rc == _lib.OK
    assert w2._L.salva_hip_particles_intersecting_compound(w2._h, t, q, comp, 0, None, None, None) == _lib.E_INVALID
    assert "salva_hip_particles_intersecting_host_shape" in last_error(w2)
    assert w2._L.salva_hip_particles_intersecting_compound(w2._h, t, (C.c_float * 4)(0, 0, 0, 2), comp, 0, None, None, None) == _lib.E_INVALID
    assert w2._L.salva_hip_particles_intersecting_mesh(w2._h, t, q, 999, 0, None, None, None) == _lib.E_INVALID


class CallsTheCompoundEntries(NonPressureForce):
    def solve(self, timestep, kernel_radius, ff, fb, fluid, boundaries, densities):
        w = self.world
        t, q = (C.c_float * 3)(0, 0, 0), (C.c_float * 4)(0, 0, 0, 1)
        self.codes = [
            int(w._L.salva_hip_set_boundary_dynamic_sampling_compound(w._h, 0, self.comp, 1, 0xFFFFFFFF)),
            int(w._L.salva_hip_particles_intersecting_compound(w._h, t, q, self.comp, 0, None, None, None)),
            int(w._L.salva_hip_particles_intersecting_mesh(w._h, t, q, self.mesh, 0, None, None, None)),
            int(w._L.salva_hip_set_boundary_dynamic_sampling_mesh(w._h, 0, self.mesh, 1, 0xFFFFFFFF)),
        ]
        self.message = last_error(w)


def test_calls_inside_a_force_callback_and_in_a_decomposed_world_are_refused():
    tet = CS.tetra()
    w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    f = Fluid(scenes.cube_fluid_positions(5, 5, 5, RAD), RAD, 1000.0)
    force = CallsTheCompoundEntries()
    force.world = w
    f.nonpressure_forces.append(force)
    w.add_fluid(f)
    w.sync_to_device()
    force.mesh = sampling.Mesh(tet[1], tet[2], oriented=True).handle(w)
    rc, force.comp = _create(w, [_part(), _part(kind=_lib.SHAPE_MESH, mesh=force.mesh)])
    assert rc == _lib.OK
    w.step(DT, GRAVITY)
    assert force.codes == [_lib.E_INVALID] * 4 and "force callback" in force.message
    assert w._L.salva_hip_num_boundaries(w._h) == 0

    pos = scenes.cube_fluid_positions(16, 6, 6, RAD)
    w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    w.add_fluid(Fluid(pos, RAD, 1000.0))
    comm = dist.Comm.loopback(1)[0]
    cx = dist.cell_x(pos, w.h())
    w.set_domain(comm, int(cx.min()), int(cx.max()), 0)
    w.step(DT, GRAVITY)
    mesh = sampling.Mesh(tet[1], tet[2], oriented=True).handle(w)
    rc, comp = _create(w, [_part(), _part(kind=_lib.SHAPE_MESH, mesh=mesh)])
    assert rc == _lib.OK
    t, q = (C.c_float * 3)(0, 0, 0), (C.c_float * 4)(0, 0, 0, 1)
    assert w._L.salva_hip_set_boundary_dynamic_sampling_compound(w._h, 0, comp, 1, 0xFFFFFFFF) == _lib.E_INVALID and "decomposed" in last_error(w)
    assert w._L.salva_hip_particles_intersecting_compound(w._h, t, q, comp, 0, None, None, None) == _lib.E_INVALID and "decomposed" in last_error(w)
    assert w._L.salva_hip_particles_intersecting_mesh(w._h, t, q, mesh, 0, None, None, None) == _lib.E_INVALID and "decomposed" in last_error(w)
    assert w._L.salva_hip_set_boundary_dynamic_sampling_mesh(w._h, 0, mesh, 1, 0xFFFFFFFF) == _lib.E_INVALID
    del w
    comm.destroy()


# ---------------------------------------------------------------------------------------------- (g) the pipeline
def _open_box(half=0.12, wall=0.02, height=0.08):
    """An open box of five cuboid slabs: a floor and four walls."""
    q = CS.ID
    return [(("cuboid", (half, wall, half)), F([0.0, -height, 0.0]), q),
            (("cuboid", (wall, height, half)), F([-(half - wall), wall, 0.0]), q), (("cuboid", (wall, height, half)), F([half - wall, wall, 0.0]), q),
            (("cuboid", (half, height, wall)), F([0.0, wall, -(half - wall)]), q), (("cuboid", (half, height, wall)), F([0.0, wall, half - wall]), q)]


def test_pipeline_with_a_compound_body():
    """A light open box dropped onto a block of fluid through FluidsPipeline: it is slowed by the fluid and carries points on its parts."""
    p = FluidsPipeline(RAD, 2.0)
    n = 12
    pos = scenes.cube_fluid_positions(n, n, n, RAD)
    pos[:, 1] += F(n * RAD)
    fl = Fluid(pos, RAD, 1000.0)
    fl.nonpressure_forces.append(XSPHViscosity(0.5, 0.5))
    p.liquid_world.add_fluid(fl)
    b = p.liquid_world.add_boundary(Boundary(np.zeros((0, 3), F)))
    parts = _open_box()
    body = RigidBody(translation=F([0.0, 2 * n * RAD + 0.12, 0.0]), linvel=F([0.0, -1.0, 0.0]), mass=1.5, principal_inertia=F([0.02, 0.02, 0.02]), dynamic=True)
    p.coupling.register_coupling(b, "box", body, DynamicContactSampling(CR.to_compound(parts)))
    most, v_free, off = 0, -1.0, 0.0
    for _ in range(40):
        p.step(GRAVITY, DT)
        if b.num_particles():  # every boundary point lies on the surface of some part (the body has not moved on yet)
            pts = np.array(b.positions, F)
            off = max(off, float(np.abs(CR.project(parts, body, pts)[0] - pts).max()))
        body.integrate(DT, GRAVITY)
        v_free += GRAVITY[1] * DT
        most = max(most, b.num_particles())
    print("box at", body.translation, "velocity", body.linvel, "free fall would be", v_free, "most points", most)
    assert most > 100 and np.isfinite(fl.positions).all() and np.isfinite(body.translation).all()
    assert body.linvel[1] > v_free + 0.3, "the fluid did not push back on the compound body"
    assert off < 1e-5, f"a boundary point is {off:.2e} off the compound's surface"


def test_cpp_mirror_compound_example():
    """examples/compound3.cpp: an open box of five slabs through include/salva_hip.hpp's `salva::Compound` and
    `Boundary::dynamic_compound`.  The box ends above the pool's floor, carried by a non-zero upward force."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "compound3"], check=True, capture_output=True)
    out = subprocess.run([os.path.join(ROOT, "examples", "compound3"), "200"], check=True, capture_output=True, text=True, timeout=300).stdout
    print(out)
    rows = [re.search(r"step (\d+): box y ([0-9.e+-]+) vy ([0-9.e+-]+), force \(([0-9.e+-]+), ([0-9.e+-]+), ([0-9.e+-]+)\).* (\d+) samples, (\d+) fluid particles inside, "
                      r"dcs passes (\d+) waits (\d+)", l) for l in out.strip().splitlines()]
    assert len(rows) == 4 and all(rows), out
    last = rows[-1]
    assert np.isfinite([float(x) for x in last.groups()]).all(), out
    assert float(last.group(2)) > 0.025 + 0.08, out   # the box's centre is above the floor by more than its own depth
    assert float(last.group(5)) > 0.0, out            # the fluid pushes it up
    assert int(last.group(7)) > 100, out              # ... through the points it carries on its slabs
    assert int(last.group(9)) == 1, out               # one pass over the fluid per step
