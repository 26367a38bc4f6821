"""Deleting particles by region on the device (salva_hip_delete_particles_in_region, the sinks of salva_hip_step)
against the f64 reading of tests/sink_reading.py and against salva_hip_delete_particles with the same mask.  The clouds hold no point
within 1e-3 r of a decision surface, so count, mask and every compacted array are compared exactly, in every case."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import sink_reading as S
from salva_amd import (Akinci2013SurfaceTension, Becker2009Elasticity, Boundary, DFSPHSolver, Fluid, IISPHSolver, LiquidWorld,
                       NonPressureForce, XSPHViscosity, _lib, dist, regions, sampling, scenes)

pytestmark = pytest.mark.gpu

F = np.float32
R = S.R
DT = 1.0 / 200.0
G = (0.0, -9.81, 0.0)
U8P = C.POINTER(C.c_uint8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def last_error(w):
    return w._L.salva_hip_last_error().decode()


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def dev_state(w, slot):
    """Every per-particle array of fluid `slot` as the device holds it."""
    lib, h = w._L, w._h
    n = int(lib.salva_hip_fluid_len(h, slot))
    out = dict(pos=np.zeros((n, 3), F), vel=np.zeros((n, 3), F), dv=np.zeros((n, 3), F), pressure=np.zeros(n, F), volume=np.zeros(n, F),
               acc=np.zeros((n, 3), F))
    if n:
        _lib.check(lib.salva_hip_get_fluid(h, slot, fp(out["pos"]), fp(out["vel"])))
        for key, field in (("dv", _lib.FIELD_VELOCITY_CHANGE), ("pressure", _lib.FIELD_PRESSURE), ("volume", _lib.FIELD_VOLUME),
                           ("acc", _lib.FIELD_ACCELERATION)):
            _lib.check(lib.salva_hip_get_fluid_field(h, slot, field, fp(out[key])))
    return out


def delete_in(w, region, slot, n_mask):
    """The raw call: (return value, mask)."""
    r = region._struct(w)
    mask = np.full(max(n_mask, 1), 7, np.uint8)
    k = int(w._L.salva_hip_delete_particles_in_region(w._h, C.byref(r), slot, mask.ctypes.data_as(U8P)))
    return k, mask[:n_mask]


def delete_mask(w, slot, mask):
    m = np.ascontiguousarray(mask, np.uint8)
    kept = int(w._L.salva_hip_delete_particles(w._h, slot, m.ctypes.data_as(U8P)))
    assert kept >= 0, last_error(w)
    return kept


# ------------------------------------------------------------------------------------------------ 1. every kind
SIZES = (1500, 2603)


@functools.lru_cache(maxsize=None)
def clouds(name):
    return tuple(S.cloud(S.REGIONS[name], n, (0.0, R), seed=11 + k) for k, n in enumerate(SIZES))


def two_fluids(name):
    """Two fluids around the region with distinct velocities, volumes, accelerations, velocity changes and pressures."""
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    fluids = []
    for k, pos in enumerate(clouds(name)):
        n = len(pos)
        f = Fluid(pos, R, 1000.0)
        i = np.arange(n, dtype=F)
        f.velocities = np.stack([i + F(0.25 + k), -i, i * F(0.5)], axis=1).astype(F)
        f.volumes = (F(1e-4) * (F(1.0) + i / F(n))).astype(F)
        f.accelerations = np.stack([i * F(0.125), i + F(k), -i], axis=1).astype(F)
        fluids.append(w.add_fluid(f))
    w.sync_to_device()
    for k, f in enumerate(fluids):
        i = np.arange(f.num_particles(), dtype=F)
        dv = np.stack([i + F(0.5), i * F(2.0) + F(k), -i - F(1.0)], axis=1).astype(F)
        _lib.check(w._L.salva_hip_set_fluid_field(w._h, f._slot, _lib.FIELD_VELOCITY_CHANGE, fp(np.ascontiguousarray(dv))))
        _lib.check(w._L.salva_hip_set_fluid_field(w._h, f._slot, _lib.FIELD_PRESSURE, fp(np.ascontiguousarray(i + F(3.0)))))
    return w, fluids


@pytest.mark.parametrize("target", ["one", "all"])
@pytest.mark.parametrize("margin", [0.0, R])
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("name", sorted(S.REGIONS))
def test_every_kind_matches_the_reading_and_numpy_compaction(name, invert, margin, target):
    w, fluids = two_fluids(name)
    before = [dev_state(w, f._slot) for f in fluids]
    assert all(same(b["pos"], c) for b, c in zip(before, clouds(name)))
    region = S.to_api(S.REGIONS[name], margin, invert)
    scope = [1] if target == "one" else [0, 1]
    want = [S.selected(S.REGIONS[name], before[k]["pos"], margin, invert) if k in scope else np.zeros(SIZES[k], bool) for k in range(2)]
    k, mask = delete_in(w, region, fluids[1]._slot if target == "one" else _lib.ALL_FLUIDS, sum(SIZES[s] for s in scope))
    assert k == sum(int(want[s].sum()) for s in scope), (k, last_error(w))
    assert 0 < k < sum(SIZES[s] for s in scope)
    assert (mask.astype(bool) == np.concatenate([want[s] for s in scope])).all() and set(np.unique(mask)) <= {0, 1}
    for s in range(2):
        after = dev_state(w, s)
        for key, old in before[s].items():
            assert same(after[key], old[~want[s]]), (s, key)


# ------------------------------------------------------------------------------------------------ 2. the edges of the scan
def sink_constants():
    text = open(os.path.join(ROOT, "salva_amd", "csrc", "sink.h")).read()
    return tuple(int(re.search(r"constexpr uint32_t %s = (\d+);" % k, text).group(1)) for k in ("SINK_ROWS", "SINK_SCAN_SPAN"))


ROWS, SPAN = sink_constants()
CARRY = ROWS * SPAN + 1
assert CARRY <= 300000
BOX = ("aabb", F([-0.5, -0.5, -0.5]), F([0.5, 0.5, 0.5]))


@pytest.mark.parametrize("pattern", ["random", "nothing", "all", "first", "last"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, ROWS - 1, ROWS, ROWS + 1, CARRY])
def test_scan_edges(n, pattern):
    rng = np.random.default_rng(n)
    inside = {"random": rng.random(n) < 0.37, "nothing": np.zeros(n, bool), "all": np.ones(n, bool)}.get(pattern)
    if inside is None:
        inside = np.zeros(n, bool)
        inside[0 if pattern == "first" else n - 1] = True
    pos = (rng.random((n, 3)) * 0.8 - 0.4).astype(F)      # in the box, 0.1 from its faces
    pos[~inside, 0] += F(1.5)                             # ... or a box width away from it
    assert (S.selected(BOX, pos, 0.0) == inside).all() and not S.in_band(BOX, pos, 0.0).any()
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    f = Fluid(pos, R, 1000.0)
    i = np.arange(n, dtype=F)  # (exact in f32: n < 2^24)
    f.velocities = np.stack([i, -i, i + F(0.5)], axis=1).astype(F)
    w.add_fluid(f)
    w.sync_to_device()
    k, mask = delete_in(w, S.to_api(BOX), 0, n)
    assert k == int(inside.sum()), (k, last_error(w))
    assert (mask.astype(bool) == inside).all()
    after = dev_state(w, 0)
    assert same(after["pos"], pos[~inside]) and same(after["vel"], f._velocities[~inside])
    if pattern == "all":
        assert w._L.salva_hip_fluid_len(w._h, 0) == 0
        w._compact_mirror(f, inside)
        st = w.step(DT, G)  # an empty fluid: the world still steps
        assert st.nparticles == 0
        f.add_particles(F([[0.0, 0.0, 0.0], [0.3, 0.0, 0.0]]))
        assert w.step(DT, G).nparticles == 2


# ------------------------------------------------------------------------------------------------ 3. the same world afterwards
def dam_break(solver, force):
    w = LiquidWorld(solver(), R, 2.0)
    pos = scenes.cube_fluid_positions(16, 16, 16, R)  # 4096 particles
    pos[:, 1] += F(16 * R + 2 * R)
    f = Fluid(scenes.jitter(pos, 0.05 * R), R, 1000.0)
    f.nonpressure_forces.append(force())
    w.add_fluid(f)
    w.add_boundary(Boundary(scenes.plane_lattice(40, 40, 0.0, R, -20 * 2 * R, -20 * 2 * R)))
    return w, f


def run_state(w, f):
    st = dev_state(w, f._slot)
    nf = np.zeros(len(st["pos"]), F)
    nb = np.zeros(len(st["pos"]), F)
    _lib.check(w._L.salva_hip_get_fluid_field(w._h, f._slot, _lib.FIELD_NUM_FLUID_CONTACTS, fp(nf)))
    _lib.check(w._L.salva_hip_get_fluid_field(w._h, f._slot, _lib.FIELD_NUM_BOUNDARY_CONTACTS, fp(nb)))
    return st, nf, nb


@pytest.mark.parametrize("solver, force", [(DFSPHSolver, lambda: XSPHViscosity(0.5, 0.5)), (IISPHSolver, lambda: Akinci2013SurfaceTension(1.0, 0.5)),
                                           (DFSPHSolver, lambda: Becker2009Elasticity(5e5, 0.3, True))], ids=["dfsph-xsph", "iisph-akinci", "dfsph-becker"])
def test_the_world_afterwards_is_the_world_after_delete_particles(solver, force):
    (a, fa), (b, fb), (c, fc), (d, fd) = (dam_break(solver, force) for _ in range(4))
    for w in (a, b, c, d):
        for _ in range(3):
            w.step(DT, G)
    corner = regions.Aabb([-1.0, 0.0, -1.0], [0.0, 0.5 * 16 * 2 * R, 0.0], margin=R)  # a quarter of the block's lower half
    n = fa.num_particles()
    k, mask = delete_in(a, corner, 0, n)
    assert 200 < k < n - 200, (k, last_error(a))
    a._compact_mirror(fa, mask.astype(bool))
    assert delete_mask(b, 0, mask) == n - k
    b._compact_mirror(fb, mask.astype(bool))
    nowhere = regions.HalfSpace([0.0, -5.0, 0.0], [0.0, 1.0, 0.0])
    k0, mask0 = delete_in(c, nowhere, _lib.ALL_FLUIDS, n)
    assert k0 == 0 and not mask0.any()
    for first, second, ffirst, fsecond in ((a, b, fa, fb), (c, d, fc, fd)):
        for step in range(3):
            s1, s2 = first.step(DT, G), second.step(DT, G)
            assert (s1.n_divergence_iters, s1.n_pressure_iters, s1.ncontacts, s1.nparticles) == \
                   (s2.n_divergence_iters, s2.n_pressure_iters, s2.ncontacts, s2.nparticles), step
            (x, xf, xb), (y, yf, yb) = run_state(first, ffirst), run_state(second, fsecond)
            assert same(x["pos"], y["pos"]) and same(x["vel"], y["vel"]) and same(x["dv"], y["dv"]) and same(x["pressure"], y["pressure"]), step
            assert (xf == yf).all() and (xb == yb).all(), step
    assert fa.num_particles() == n - k and len(fa.positions) == n - k


# ------------------------------------------------------------------------------------------------ 4. sinks
SHEET = ("cuboid", (0.15, 0.0125, 0.15))   # one layer of particles, well inside the cylinder ...
SPRAY = ("cuboid", (0.05, 0.0125, 0.05))   # ... and one well outside it
NOZZLE, ASIDE = F([0.0, 0.6, 0.0]), F([0.6, 0.6, 0.0])
FLOOR = ("halfspace", F([0.0, 0.45, 0.0]), F([0.0, 1.0, 0.0]))
WELL = ("shape", ("cylinder", 1.9, 0.31), F([0.0, 0.0, 0.0]), F([0.0, 0.0, 0.0, 1.0]))


def faucet_world():
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    f = Fluid(np.zeros((0, 3), F), R, 1000.0)
    f.nonpressure_forces.append(XSPHViscosity(0.5, 0.0))
    w.add_fluid(f)
    w.sync_to_device()
    return w, f


def test_sinks_in_the_step_against_the_host_loop():
    """40 steps of a faucet: a sheet every 10 steps, a half-space below and an inverted cylinder around as sinks, against a twin that
    reads the positions, takes its masks from the f64 reading and calls salva_hip_delete_particles before every step.  Every emission is
    one layer of particles - its particles keep one common height, so a sheet meets the plane in one step - in two pieces: one stays
    0.06 inside the cylinder while it spreads, the other starts 0.19 outside it and is gone at the next step entry.  No particle comes
    within the band of either surface at a step entry; the loop asserts that on the twin's positions."""
    (w, f), (t, ft) = faucet_world(), faucet_world()
    floor = w.add_sink(S.to_api(FLOOR), f)
    well = w.add_sink(S.to_api(WELL, invert=True), f)
    assert (floor, well) == (0, 1)
    deleted = {floor: 0, well: 0}
    lib = w._L
    for step in range(40):
        if step % 10 == 0:
            added = [x.add_particles_from_shape(SHEET, NOZZLE, velocity=(0.0, -1.0, 0.0)) + x.add_particles_from_shape(SPRAY, ASIDE, velocity=(0.0, -1.0, 0.0))
                     for x in (f, ft)]
            assert added[0] == added[1] > 40
        last = {}
        for sink, (region, invert) in ((floor, (FLOOR, False)), (well, (WELL, True))):  # the twin, in handle order
            n = int(lib.salva_hip_fluid_len(t._h, 0))
            p = dev_state(t, 0)["pos"]
            assert not S.in_band(region, p, 0.0).any(), (step, sink)
            m = S.selected(region, p, 0.0, invert)
            last[sink] = int(m.sum())
            if m.any():
                assert delete_mask(t, 0, m) == n - last[sink]
                t._compact_mirror(ft, m)
        s1, s2 = w.step(DT, G), t.step(DT, G)
        assert s1.nparticles == s2.nparticles and (s1.n_divergence_iters, s1.n_pressure_iters, s1.ncontacts) == \
               (s2.n_divergence_iters, s2.n_pressure_iters, s2.ncontacts), step
        assert lib.salva_hip_fluid_len(w._h, 0) == lib.salva_hip_fluid_len(t._h, 0) == f.num_particles(), step
        x, y = dev_state(w, 0), dev_state(t, 0)
        assert all(same(x[key], y[key]) for key in ("pos", "vel", "dv", "pressure", "volume")), step
        for sink in (floor, well):
            deleted[sink] += last[sink]
            assert w.sink_stats(sink) == (last[sink], deleted[sink]), (step, sink)
    assert deleted[floor] > 30 and deleted[well] > 10  # both fired
    assert same(f.positions, ft.positions) and len(f.velocities) == f.num_particles()


def test_sink_pose_removal_and_ownership():
    pos = scenes.cube_fluid_positions(12, 12, 12, R)  # at rest spacing and without gravity: nothing moves between the steps
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    f = w.add_fluid(Fluid(pos, R, 1000.0))
    ball = ("shape", ("ball", 0.2), F([5.0, 5.0, 5.0]), F([0, 0, 0, 1]))
    sink = w.add_sink(S.to_api(ball), f)
    zero = (0.0, 0.0, 0.0)
    w.step(1e-4, zero)
    assert w.sink_stats(sink) == (0, 0) and f.num_particles() == 1728
    for centre in ([0.0137, 0.0071, -0.0113], [0.2237, 0.1571, -0.0613]):  # the next step deletes at the new place
        w.set_sink_pose(sink, centre)
        before = dev_state(w, 0)
        here = ("shape", ("ball", 0.2), F(centre), F([0, 0, 0, 1]))
        assert not S.in_band(here, before["pos"], 0.0).any()
        want = S.selected(here, before["pos"], 0.0)
        total = w.sink_stats(sink)[1]
        w.step(1e-4, zero)
        assert w.sink_stats(sink) == (int(want.sum()), total + int(want.sum())) and want.sum() > 10
        assert f.num_particles() == len(before["pos"]) - int(want.sum()) == len(f.positions)
    assert w._L.salva_hip_set_sink_pose(w._h, sink, fp(F([0, 0, 0])), fp(F([0, 0, 0, 2]))) == _lib.E_INVALID
    # a removed sink deletes nothing
    w.set_sink_pose(sink, [-0.2, -0.1, 0.05])
    w.remove_sink(sink)
    n = f.num_particles()
    w.step(1e-4, zero)
    assert f.num_particles() == n == w._L.salva_hip_fluid_len(w._h, 0)
    assert w._L.salva_hip_remove_sink(w._h, sink) == _lib.E_INVALID and w._L.salva_hip_get_sink_stats(w._h, sink, (C.c_uint64 * 2)()) == _lib.E_INVALID
    # a sink shares ownership of its mesh and of its compound
    mesh_region = S.to_api(S.REGIONS["mesh"])
    compound_region = S.to_api(S.REGIONS["compound"])
    s1, s2 = w.add_sink(mesh_region, f), w.add_sink(compound_region)
    assert s1 == sink  # (the freed handle is given out again)
    mesh, compound = mesh_region.mesh.handle(w), compound_region.compound.handle(w)
    assert w._L.salva_hip_destroy_mesh(w._h, mesh) == _lib.E_INVALID and "sink" in last_error(w)
    assert w._L.salva_hip_destroy_compound(w._h, compound) == _lib.E_INVALID and "sink" in last_error(w)
    assert w._L.salva_hip_set_sink_pose(w._h, s2, fp(F([0.5, 0, 0])), fp(F([0, 0, 0, 1]))) == _lib.OK
    w.step(1e-4, zero)
    w.remove_sink(s1)
    w.remove_sink(s2)
    assert w._L.salva_hip_destroy_mesh(w._h, mesh) == _lib.OK and w._L.salva_hip_destroy_compound(w._h, compound) == _lib.OK
    w.step(1e-4, zero)


# ------------------------------------------------------------------------------------------------ 5. refusals
class CallsTheRegionEntries(NonPressureForce):
    codes = None

    def solve(self, timestep, kernel_radius, ff, fb, fluid, boundaries, densities):
        w, r, h = self.world, regions.Aabb([-1, -1, -1], [1, 1, 1])._struct(None), C.c_uint32(0)
        self.codes = [int(w._L.salva_hip_delete_particles_in_region(w._h, C.byref(r), 0, None)), int(w._L.salva_hip_add_sink(w._h, C.byref(r), 0, C.byref(h)))]
        self.message = last_error(w)


def small_world():
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    f = w.add_fluid(Fluid(scenes.cube_fluid_positions(5, 5, 5, R), R, 1000.0))
    w.sync_to_device()
    return w, f


def test_every_refusal_leaves_a_world_that_steps():
    w, f = small_world()
    n = f.num_particles()
    good = regions.Shape(("ball", 0.5))._struct(w)
    surface = sampling.Mesh(S.OCTA_V, S.OCTA_I, oriented=False)
    solid = sampling.Mesh(S.OCTA_V, S.OCTA_I, oriented=True)
    id4 = F([0, 0, 0, 1])
    open_compound = sampling.Compound([(("ball", 0.1), F([0, 0, 0]), id4), (surface, F([0.5, 0, 0]), id4)])

    def edit(base, **kw):
        r = type(base)()
        C.memmove(C.byref(r), C.byref(base), C.sizeof(r))
        for key, value in kw.items():
            if isinstance(value, (list, tuple)):
                getattr(r, key)[:] = value
            else:
                setattr(r, key, value)
        return r

    hs = regions.HalfSpace([0, 0, 0], [0, 1, 0])._struct(w)
    box = regions.Aabb([-1, -1, -1], [1, 1, 1])._struct(w)
    bad_shape, neg_shape = edit(good), edit(good)
    bad_shape.shape.kind = 42
    neg_shape.shape.params[0] = -1.0
    cases = {
        "struct_size": edit(good, struct_size=64), "version": edit(good, version=2), "flag": edit(good, flags=2),
        "kind 0": edit(good, kind=0), "kind 99": edit(good, kind=99),
        "mesh handle": edit(good, kind=_lib.REGION_MESH, handle=77), "compound handle": edit(good, kind=_lib.REGION_COMPOUND, handle=77),
        "rotation": edit(good, rotation_ijkw=[0, 0, 0, 2]), "nan rotation": edit(good, rotation_ijkw=[float("nan"), 0, 0, 1]),
        "translation": edit(good, translation=[float("inf"), 0, 0]),
        "normal": edit(hs, normal=[0, 2, 0]), "nan point": edit(hs, point=[0, float("nan"), 0]),
        "negative margin": edit(good, margin=-1e-3), "nan margin": edit(hs, margin=float("nan")), "inf margin": edit(box, margin=float("inf")),
        "shape kind": bad_shape, "shape params": neg_shape,
        "mins > maxs": edit(box, mins=[0, 2, 0]), "nan box": edit(box, maxs=[1, float("nan"), 1]),
        "open mesh": regions.Mesh(surface)._struct(w), "open compound": regions.Compound(open_compound)._struct(w),
        "mesh rotation": edit(regions.Mesh(solid)._struct(w), rotation_ijkw=[0, 0, 1, 1]),
    }
    lib, h = w._L, C.c_uint32(0)
    for what, r in cases.items():
        assert lib.salva_hip_delete_particles_in_region(w._h, C.byref(r), 0, None) == _lib.E_INVALID, what
        assert last_error(w), what
        assert lib.salva_hip_add_sink(w._h, C.byref(r), 0, C.byref(h)) == _lib.E_INVALID, what
        assert w.step(DT, G).nparticles == n, what
    assert lib.salva_hip_delete_particles_in_region(w._h, C.byref(good), 3, None) == _lib.E_INVALID  # no such fluid
    assert lib.salva_hip_add_sink(w._h, C.byref(good), 3, C.byref(h)) == _lib.E_INVALID
    assert lib.salva_hip_delete_particles_in_region(w._h, None, 0, None) == _lib.E_INVALID
    assert lib.salva_hip_set_sink_pose(w._h, 0, fp(F([0, 0, 0])), fp(id4)) == _lib.E_INVALID and "no such sink" in last_error(w)
    plane_sink = w.add_sink(regions.HalfSpace([0, -5, 0], [0, 1, 0]))
    assert lib.salva_hip_set_sink_pose(w._h, plane_sink, fp(F([0, 0, 0])), fp(id4)) == _lib.E_INVALID  # a half-space has no pose
    assert w.step(DT, G).nparticles == n and f.num_particles() == n

    # inside a force callback, inside a coupling callback
    w, f = small_world()
    force = CallsTheRegionEntries()
    force.world = w
    f.nonpressure_forces.append(force)
    w.step(DT, G)
    assert force.codes == [_lib.E_INVALID, _lib.E_INVALID] and "force callback" in force.message
    f.nonpressure_forces.clear()
    seen = []

    def coupling(_user, _world, phase, dt):
        r = regions.Aabb([-1, -1, -1], [1, 1, 1])._struct(None)
        seen.append((int(w._L.salva_hip_delete_particles_in_region(w._h, C.byref(r), 0, None)), last_error(w)))
        return 0

    cb = _lib.COUPLING_CALLBACK(coupling)
    _lib.check(w._L.salva_hip_set_coupling_callback(w._h, cb, None))
    w.step(DT, G)
    _lib.check(w._L.salva_hip_set_coupling_callback(w._h, _lib.COUPLING_CALLBACK(), None))
    assert [c for c, _ in seen] == [_lib.E_INVALID, _lib.E_INVALID] and all("coupling callback" in m for _, m in seen)
    assert w.step(DT, G).nparticles == f.num_particles() == 125
    assert w.delete_particles_in(regions.Aabb([-1, -1, -1], [1, 1, 1])) == 125  # (outside the callbacks the same call works)

    # a decomposed world
    pos = scenes.cube_fluid_positions(16, 6, 6, R)
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    w.add_fluid(Fluid(pos, R, 1000.0))
    comm = dist.Comm.loopback(1)[0]
    cx = dist.cell_x(pos, w.h())
    w.set_domain(comm, int(cx.min()), int(cx.max()), 0)
    r, h = regions.Aabb([-1, -1, -1], [1, 1, 1])._struct(None), C.c_uint32(0)
    assert w._L.salva_hip_add_sink(w._h, C.byref(r), 0, C.byref(h)) == _lib.E_INVALID and "decomposed" in last_error(w)
    w.step(DT, G)
    assert w._L.salva_hip_delete_particles_in_region(w._h, C.byref(r), 0, None) == _lib.E_INVALID and "salva_hip_delete_owned" in last_error(w)
    assert w._L.salva_hip_add_sink(w._h, C.byref(r), 0, C.byref(h)) == _lib.E_INVALID
    assert w.step(DT, G).nparticles == len(pos)
    del w
    comm.destroy()


# ------------------------------------------------------------------------------------------------ 6. the Python mirror
def test_python_mirror_follows_the_device():
    name = "cylinder"
    region = S.REGIONS[name]
    pos = clouds(name)[1]
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    vel = np.stack([np.arange(len(pos), dtype=F)] * 3, axis=1)
    f, other = Fluid(pos, R, 1000.0), Fluid(clouds(name)[0], R, 1000.0)
    f.velocities = vel
    vol = (f.volumes * (F(1.0) + F(0.1) * np.arange(len(pos), dtype=F) / F(len(pos)))).astype(F)
    f.volumes = vol
    w.add_fluid(other)
    w.add_fluid(f)
    want = S.selected(region, pos, R, True)  # everything outside the cylinder
    pending = int(np.flatnonzero(~want)[0])
    f.delete_particle_at_next_timestep(pending)  # (stays pending through the calls)
    assert w.delete_particles_in(S.to_api(region, R, True), f) == int(want.sum())
    assert other.num_particles() == SIZES[0] and len(f._deleted) == len(pos) - int(want.sum()) and f._deleted.sum() == 1
    assert same(f.positions, pos[~want]) and same(f.velocities, vel[~want]) and same(f.volumes, vol[~want]) and len(f.accelerations) == f.num_particles()
    first = ("shape", ("ball", 0.12), F([0.2, -0.05, 0.15]), F([0, 0, 0, 1]))  # ... then a ball out of every fluid
    all_want = [S.selected(first, x.positions, 0.0) for x in (other, f)]
    assert not any(S.in_band(first, x.positions, 0.0).any() for x in (other, f)) and all(m.sum() > 3 for m in all_want)
    kept = [x.positions[~m].copy() for x, m in zip((other, f), all_want)]
    assert w.delete_particles_in(S.to_api(first)) == sum(int(m.sum()) for m in all_want)
    assert same(other.positions, kept[0]) and same(f.positions, kept[1]) and f._deleted.sum() == 1
    # a step with a sink: the pending deletion goes first, the sink takes what the reading says of the positions at step entry
    w.sync_to_device()
    assert f._deleted.sum() == 0 and f.num_particles() == len(kept[1]) - 1
    entry, entry_vol = f.positions.copy(), f.volumes.copy()
    ball = ("shape", ("ball", 0.15), F([0.0, -0.1, 0.15]), F([0, 0, 0, 1]))
    assert not S.in_band(ball, entry, 0.0).any()
    hit = S.selected(ball, entry, 0.0)
    assert hit.sum() > 5
    sink = w.add_sink(S.to_api(ball), f)
    n_other = other.num_particles()
    w.step(1e-4, (0.0, 0.0, 0.0))
    assert w.sink_stats(sink) == (int(hit.sum()), int(hit.sum()))
    assert f.num_particles() == len(entry) - int(hit.sum()) == len(f.positions) == len(f.velocities) == len(f._deleted) == len(f.volumes)
    assert other.num_particles() == n_other == len(other.positions)
    got = dev_state(w, f._slot)
    assert same(f.positions, got["pos"]) and same(f.velocities, got["vel"])
    assert same(f.volumes, entry_vol[~hit]) and same(f.volumes, got["volume"])  # the survivors, in order


# ------------------------------------------------------------------------------------------------ 7. the C++ example
def test_cpp_example_runs_the_faucet_without_reading_positions():
    """examples/faucet_sink3.cpp: faucet3's scene with a sampled nozzle and two sinks through include/salva_hip.hpp.  After 100 steps
    the inverted cylinder has taken what ran off the plate, the half-space what fell below it, and the books balance."""
    import subprocess

    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "faucet_sink3"], check=True, capture_output=True)
    out = subprocess.run([os.path.join(ROOT, "examples", "faucet_sink3"), "100"], check=True, capture_output=True, text=True, timeout=120).stdout
    print(out)
    m = re.search(r"step 100: (\d+) particles \(added (\d+), sinks took (\d+) below and (\d+) around\)", out)
    assert m, out
    left, added, below, around = (int(x) for x in m.groups())
    assert added > 0 and left + below + around == added, out
    y = re.search(r"y in \[([0-9.e+-]+), ([0-9.e+-]+)\]", out)
    assert y and float(y.group(1)) > -0.3 - 0.1, out  # nothing far below the plane: a step moves a particle by centimetres at most


# ------------------------------------------------------------------------------------------------ 8. the sorted working set
# After a step the current positions are the sorted working set, and the predicates walk them there (per-fluid tally through the sorted
# model array), then again in host order for the flags.  The particles below lie more than a kernel radius apart and start at rest
# without gravity: nothing acts on them, a step leaves them where they are, and what they are compared with is read from the device.
ZERO = (0.0, 0.0, 0.0)
SPACING = 0.11  # > h = 4 r = 0.1, jitter included


def sparse_lattice(side, centre, seed, jitter=0.004):
    i, j, k = side if isinstance(side, tuple) else (side, side, side)
    g = np.stack(np.meshgrid(np.arange(i), np.arange(j), np.arange(k), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    g = (g - (np.array([i, j, k]) - 1) / 2.0) * SPACING + np.asarray(centre, np.float64)
    rng = np.random.default_rng(seed)
    return (g + (rng.random(g.shape) * 2.0 - 1.0) * jitter).astype(F), rng


def raw_step(w, dt=1e-4, g=ZERO):
    st = _lib.StepStats()
    _lib.check(w._L.salva_hip_step(w._h, dt, (C.c_float * 3)(*g), C.byref(st)))
    return st


@functools.lru_cache(maxsize=None)
def sparse_clouds(name):
    region = S.REGIONS[name]
    lo, hi = S.bounds(region)
    pool, rng = sparse_lattice(17, 0.5 * (lo + hi), seed=23)
    pool = pool[rng.permutation(len(pool))]
    pool = pool[~(S.in_band(region, pool, 0.0) | S.in_band(region, pool, R))]
    assert len(pool) >= sum(SIZES) and np.abs(pool).max() < 2.0
    return np.ascontiguousarray(pool[:SIZES[0]]), np.ascontiguousarray(pool[SIZES[0]:sum(SIZES)])


@pytest.mark.parametrize("target", ["one", "all"])
@pytest.mark.parametrize("invert, margin", [(False, R), (True, 0.0)])
@pytest.mark.parametrize("name", sorted(S.REGIONS))
def test_every_kind_on_the_sorted_working_set(name, invert, margin, target):
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    fluids = []
    for k, pos in enumerate(sparse_clouds(name)):
        f = Fluid(pos, R, 1000.0)
        f.volumes = (f.volumes * (F(1.0) + F(0.25) * np.arange(len(pos), dtype=F) / F(len(pos)))).astype(F)
        fluids.append(w.add_fluid(f))
    w.sync_to_device()
    raw_step(w)
    before = [dev_state(w, s) for s in range(2)]
    raw_step(w)  # (reading the state refreshed the host-order arrays: the step makes the sorted set the current one again)
    assert all(same(dev_pos, b["pos"]) for dev_pos, b in zip(sparse_clouds(name), before))  # nothing acted on them
    region = S.REGIONS[name]
    assert not any(S.in_band(region, b["pos"], margin).any() for b in before)
    scope = [1] if target == "one" else [0, 1]
    want = [S.selected(region, before[k]["pos"], margin, invert) if k in scope else np.zeros(SIZES[k], bool) for k in range(2)]
    k, mask = delete_in(w, S.to_api(region, margin, invert), 1 if target == "one" else _lib.ALL_FLUIDS, sum(SIZES[s] for s in scope))
    assert k == sum(int(want[s].sum()) for s in scope), (k, last_error(w))
    assert 0 < k < sum(SIZES[s] for s in scope)
    assert (mask.astype(bool) == np.concatenate([want[s] for s in scope])).all() and set(np.unique(mask)) <= {0, 1}
    for s in range(2):
        after = dev_state(w, s)
        for key in ("pos", "vel", "volume"):  # (velocity changes and pressures are the last step's own: section 1 and 3 compare them)
            assert same(after[key], before[s][key][~want[s]]), (s, key)
    assert raw_step(w).nparticles == sum(SIZES) - k


def test_mask_from_the_sorted_working_set_where_the_second_level_carries():
    """CARRY rows after a step, with the mask: the flags are written twice (sorted order, then host order) before the mask is read.
    The lattice reaches +-3.6, where an f32 coordinate has an ulp of 2.4e-7 and the box distance errs by a few of them: still two
    orders below the band of 2.5e-5 the cloud keeps clear of."""
    box = ("aabb", F([-1.0, -1.0, -1.0]), F([1.0, 1.0, 1.0]))
    pool, rng = sparse_lattice((64, 64, 65), (0.0, 0.0, 0.0), seed=29)
    pool = pool[~S.in_band(box, pool, 0.0)]
    pos = np.ascontiguousarray(pool[rng.permutation(len(pool))[:CARRY]])
    assert len(pos) == CARRY and np.abs(pos).max() < 3.7
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    w.add_fluid(Fluid(pos, R, 1000.0))
    w.sync_to_device()
    raw_step(w)
    want = S.selected(box, pos, 0.0)
    k, mask = delete_in(w, S.to_api(box), 0, CARRY)
    assert k == int(want.sum()) and 1000 < k < CARRY - 1000, (k, last_error(w))
    assert (mask.astype(bool) == want).all()
    assert same(dev_state(w, 0)["pos"], pos[~want])


# ------------------------------------------------------------------------------------------------ 9. the inherited solver buffer
def test_inherited_solver_buffer_is_filtered_like_delete_particles_filters_it():
    """remove_fluid leaves the removed fluid's velocity changes behind as the slot's buffer: the fluid that moves into the slot takes
    its head, particles added before the next step its tail.  A region delete in that slot filters the buffer as
    salva_hip_delete_particles with the same mask does: the velocity changes right after, those of particles added next, and the
    next steps are bit-identical."""
    def build():
        w = LiquidWorld(DFSPHSolver(), R, 2.0)
        a = scenes.jitter(scenes.cube_fluid_positions(12, 12, 12, R), 0.05 * R)
        b = scenes.jitter(scenes.cube_fluid_positions(8, 8, 8, R), 0.05 * R, seed=7)
        b[:, 0] += F(0.8)
        for pos in (a, b):
            f = Fluid(pos, R, 1000.0)
            f.nonpressure_forces.append(XSPHViscosity(0.5, 0.0))
            w.add_fluid(f)
        w.sync_to_device()
        for _ in range(3):
            raw_step(w, DT, G)
        assert np.abs(dev_state(w, 0)["dv"]).max() > 0
        _lib.check(w._L.salva_hip_remove_fluid(w._h, 0))  # the 512 particles move into slot 0; 1728 velocity changes stay behind
        assert w._L.salva_hip_num_fluids(w._h) == 1 and w._L.salva_hip_fluid_len(w._h, 0) == 512
        return w

    x, y = build(), build()
    half = regions.Aabb([0.8, -1.0, -1.0], [2.0, 1.0, 1.0], margin=0.0)  # the far half of the block
    k, mask = delete_in(x, half, 0, 512)
    assert 100 < k < 412, (k, last_error(x))
    assert delete_mask(y, 0, mask) == 512 - k
    sx, sy = dev_state(x, 0), dev_state(y, 0)
    assert all(same(sx[key], sy[key]) for key in sx) and np.abs(sx["dv"]).max() > 0
    extra = scenes.cube_fluid_positions(10, 10, 10, R)  # 1000 more: past the buffer's filtered head, into its tail and beyond
    extra[:, 1] += F(1.0)
    for w in (x, y):
        _lib.check(w._L.salva_hip_add_particles(w._h, 0, len(extra), fp(extra), None))
    sx, sy = dev_state(x, 0), dev_state(y, 0)
    assert len(sx["dv"]) == 512 - k + 1000 and all(same(sx[key], sy[key]) for key in sx)
    assert np.abs(sx["dv"][512 - k:]).max() > 0  # the new particles did inherit something
    for step in range(2):
        s1, s2 = raw_step(x, DT, G), raw_step(y, DT, G)
        assert (s1.n_divergence_iters, s1.n_pressure_iters, s1.ncontacts) == (s2.n_divergence_iters, s2.n_pressure_iters, s2.ncontacts), step
        sx, sy = dev_state(x, 0), dev_state(y, 0)
        assert all(same(sx[key], sy[key]) for key in ("pos", "vel", "dv", "pressure")), step


# ------------------------------------------------------------------------------------------------ 10. sinks and their fluids
def test_sinks_follow_their_fluid_and_an_overlap_counts_once():
    a, _ = sparse_lattice(9, (0.0, 0.0, 0.0), seed=31)
    b, _ = sparse_lattice(9, (0.0, 0.0, 0.0), seed=37)
    b = (b + F([0.03, 0.02, 0.01])).astype(F)  # (the two fluids never meet: none of this world's particles has a neighbour)
    b[:, 0] += F(1.2)
    w = LiquidWorld(DFSPHSolver(), R, 2.0)
    fa, fb = w.add_fluid(Fluid(a, R, 1000.0)), w.add_fluid(Fluid(b, R, 1000.0))
    w.sync_to_device()
    ball_a = ("shape", ("ball", 0.25), F([0.0, 0.0, 0.0]), F([0, 0, 0, 1]))
    ball_b = ("shape", ("ball", 0.25), F([1.2, 0.0, 0.0]), F([0, 0, 0, 1]))
    wide_b = ("shape", ("ball", 0.33), F([1.25, 0.0, 0.0]), F([0, 0, 0, 1]))  # overlaps ball_b
    for region, pts in ((ball_a, a), (ball_b, b), (wide_b, b), (wide_b, a)):
        assert not S.in_band(region, pts, 0.0).any()
    on_a, on_b, on_all = w.add_sink(S.to_api(ball_a), fa), w.add_sink(S.to_api(ball_b), fb), w.add_sink(S.to_api(wide_b))
    lib = w._L
    _lib.check(lib.salva_hip_remove_fluid(w._h, 0))  # the second fluid moves into slot 0 ...
    out = (C.c_uint64 * 2)()
    assert lib.salva_hip_get_sink_stats(w._h, on_a, out) == _lib.E_INVALID  # ... the first one's sink went with it ...
    raw_step(w)
    first, second = S.selected(ball_b, b, 0.0), S.selected(wide_b, b, 0.0)
    assert first.sum() > 20 and (second & ~first).sum() > 20 and (second & first).sum() > 20
    assert w.sink_stats(on_b) == (int(first.sum()), int(first.sum()))            # ... and the second one's followed it
    assert w.sink_stats(on_all) == (int((second & ~first).sum()),) * 2           # a row two sinks select counts for the first
    assert same(dev_state(w, 0)["pos"], b[~(first | second)])
    raw_step(w)
    assert w.sink_stats(on_b) == (0, int(first.sum())) and lib.salva_hip_fluid_len(w._h, 0) == int((~(first | second)).sum())
    assert w.add_sink(S.to_api(ball_a)) == on_a  # the freed handle is given out again
