"""The ray sampler on a compound (salva_amd/csrc/sample.hip k_compound_mark, raycast.h; DESIGN.md §17 "Ray sampling") against the
numpy reading (tests/compound_cast_reading.py) and against the host arm driven by the reading's cast, bit for bit; a geometric
sanity check of the reading itself; the two ways to use the samples without a host round trip; the error cases."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import compound_cast_reading as CC
import compound_reading as CR
import compound_scenes as CS
import mesh_fixtures as X
import sampling_reading as R
from salva_amd import Boundary, DFSPHSolver, Fluid, LiquidWorld, _lib, dist, scenes, sampling
from salva_amd.coupling import ColliderCouplingSet, RigidBody, StaticSampling

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAD = CC.RAD
FP = C.POINTER(C.c_float)
DT = 1.0 / 240.0
G = (0.0, -9.81, 0.0)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@functools.lru_cache(maxsize=None)
def reading(name, mode):
    _, pos, N = CC.sample(CC.SCENES[name](), RAD, mode)
    pos.setflags(write=False)
    return pos, N


@functools.lru_cache(maxsize=None)
def compound_of(name):
    return CR.to_compound(CC.SCENES[name]())


@pytest.fixture(scope="module")
def world(hip_lib):
    return LiquidWorld(DFSPHSolver(), RAD, 2.0)


def last_error(w):
    return w._L.salva_hip_last_error().decode()


# ---------------------------------------------------------------------------------------------- 1, 2. device = reading = host arm
@pytest.mark.parametrize("mode", [R.SURFACE, R.VOLUME])
@pytest.mark.parametrize("name", list(CC.SCENES))
def test_device_equals_reading_and_host_arm(world, name, mode):
    parts = CC.SCENES[name]()
    ref, N = reading(name, mode)
    got = sampling._sample(compound_of(name), RAD, mode, world)
    host = sampling._sample(sampling.HostRayShape(lambda: CR.local_aabb(parts), lambda origins, axis: CC.cast_axis(parts, origins, axis)), RAD, mode, world)
    print(name, mode, "lattice", N, "reading", len(ref), "host arm", len(host), "device", len(got))
    assert len(ref) > 100
    assert len(got) == len(ref) and np.array_equal(bits(got), bits(ref))
    assert len(host) == len(got) and np.array_equal(bits(host), bits(got))


# ---------------------------------------------------------------------------------------------- 3. the samples lie where they should
@pytest.mark.parametrize("name", list(CC.SCENES))
def test_samples_lie_within_a_spacing_of_the_compound(name):
    """f64 distances to compound_reading's projections: a surface sample within s = 2 r of some part's boundary, a volume sample
    within s of the union of the parts."""
    parts = CC.SCENES[name]()
    s = 2.0 * RAD
    for mode in (R.SURFACE, R.VOLUME):
        pts, _ = reading(name, mode)
        best = np.full(len(pts), np.inf)
        for part in parts:
            proj, inside = CR.part_project(part, np.array(pts))
            d = np.linalg.norm(pts.astype(np.float64) - proj.astype(np.float64), axis=1)
            best = np.minimum(best, d if mode == R.SURFACE else np.where(inside, 0.0, d))
        print(name, mode, "farthest sample", best.max(), "of", s)
        assert best.max() <= s


# ---------------------------------------------------------------------------------------------- 4. fluid from a posed compound
def moving_body():
    return RigidBody(translation=np.array([0.02, -0.01, 0.03], F), rotation=scenes.quat_from_scaled_axis([0.1, 0.3, -0.2]),
                     linvel=np.array([0.1, 0.0, -0.05], F), angvel=np.array([0.0, 0.4, 0.1], F), local_com=np.array([0.01, 0.0, 0.0], F),
                     mass=50.0, dynamic=True)


def test_fluid_from_a_posed_compound_equals_the_posed_samples(hip_lib):
    """pose_point of the samples is what a StaticSampling boundary of the same points shows under the same pose (the comparison of
    tests/test_sampling_gpu.py for shapes)."""
    pts, _ = reading("body_compound", R.VOLUME)
    body, vel = moving_body(), F([0.25, -1.0, 0.5])
    w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    f = w.add_fluid(Fluid([], RAD, 1000.0))
    b = w.add_boundary(Boundary([]))
    cs = ColliderCouplingSet()
    cs.register_coupling(b, "c", body, StaticSampling(pts))
    w.sync_to_device()
    cs.update_boundaries(w)
    posed = w._boundary_particles(b)[0]
    assert f.add_particles_from_shape(compound_of("body_compound"), body.translation, body.rotation, R.VOLUME, vel) == len(pts)
    assert np.array_equal(bits(f.positions), bits(posed))
    assert np.abs(posed - pts).max() > 1e-3
    assert np.array_equal(bits(f.velocities), bits(np.tile(vel, (len(pts), 1))))
    vol = np.zeros(len(pts), F)
    _lib.check(w._L.salva_hip_get_fluid_field(w._h, f._slot, _lib.FIELD_VOLUME, vol.ctypes.data_as(FP)))
    r = F(RAD)
    assert np.array_equal(bits(vol), bits(np.full(len(pts), r * r * r * F(6.4), F)))  # as salva_hip_add_particles sets them
    # surface mode, no velocity: appended behind the first batch
    spts, _ = reading("body_compound", R.SURFACE)
    assert f.add_particles_from_shape(compound_of("body_compound"), (0, 0, 0), (0, 0, 0, 1), R.SURFACE) == len(spts)
    assert np.array_equal(bits(f.positions[len(pts):]), bits(spts)) and not f.velocities[len(pts):].any()


# ---------------------------------------------------------------------------------------------- 5. boundary from a compound
def test_boundary_from_a_compound_equals_uploaded_samples(hip_lib):
    surf, _ = reading("slab_compound", R.SURFACE)
    block = R.sample(("cuboid", (0.06, 0.05, 0.07)), RAD, R.VOLUME)[1]
    fluid = (block + F([0.0, 0.16, 0.0])).astype(F)
    # the boundary's local points: what an unposed boundary shows
    w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    w.add_fluid(Fluid(fluid, RAD, 1000.0))
    b = w.add_boundary(Boundary([]))
    cs = ColliderCouplingSet()
    cs.register_coupling(b, "slabs", None, StaticSampling.from_shape(compound_of("slab_compound")))
    w.sync_to_device()
    cs.update_boundaries(w)
    assert b.num_particles() == len(surf) and np.array_equal(bits(w._boundary_particles(b)[0]), bits(surf))
    # posed by a moving body, one step: a StaticSampling boundary uploaded from the same points
    res = []
    for from_compound in (True, False):
        w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
        f = w.add_fluid(Fluid(fluid, RAD, 1000.0))
        b = w.add_boundary(Boundary([]))
        cs = ColliderCouplingSet()
        comp = CR.to_compound(CC.SCENES["slab_compound"]())
        cs.register_coupling(b, "slabs", moving_body(), StaticSampling.from_shape(comp) if from_compound else StaticSampling(surf))
        w.sync_to_device()
        cs.update_boundaries(w)
        assert b.num_particles() == len(surf)
        pos, vel = w._boundary_particles(b)
        w.step(DT, G)
        res.append((np.array(pos), np.array(vel), f.positions.copy(), f.velocities.copy(), np.array(w._boundary_particles(b)[0])))
        if from_compound:  # the boundary holds its points, not the compound
            h = comp.handle(w)
            assert w._L.salva_hip_destroy_compound(w._h, h) == _lib.OK
            assert w._L.salva_hip_destroy_compound(w._h, h) == _lib.E_INVALID  # gone
            w.step(DT, G)
            assert np.isfinite(f.positions).all()
    for a, c in zip(*res):
        assert np.array_equal(bits(a), bits(c))
    assert np.abs(res[0][1]).max() > 0 and np.abs(res[0][0] - surf).max() > 1e-3  # the pose moves


# ---------------------------------------------------------------------------------------------- 6. errors
def test_errors(world):
    w = world
    out = np.zeros((4, 3), F)
    assert w._L.salva_hip_sample_compound(w._h, 9999, RAD, 0, 0, None) == _lib.E_INVALID
    assert "no such compound" in last_error(w)
    h = compound_of("far_apart").handle(w)
    assert w._L.salva_hip_sample_compound(w._h, h, RAD, 2, 4, out.ctypes.data_as(FP)) == _lib.E_INVALID      # a bad mode
    assert w._L.salva_hip_sample_compound(w._h, h, 0.0, 0, 4, out.ctypes.data_as(FP)) == _lib.E_INVALID      # a bad radius
    assert w._L.salva_hip_sample_compound(w._h, h, float("nan"), 0, 4, out.ctypes.data_as(FP)) == _lib.E_INVALID
    assert not out.any()
    # a ray along x crosses 40 slabs 80 times
    sv, st, _ = X.slabs()
    stack = sampling.Compound([(sampling.Mesh(sv, st, oriented=True), F([0.0, 0.0, 0.0]), CS.ID)])
    with pytest.raises(_lib.SalvaHipError) as e:
        sampling._sample(stack, 0.05, R.SURFACE, w)
    assert e.value.code == _lib.E_CAPACITY and "64" in str(e.value)
    # ... and the world samples on
    got = sampling.shape_surface_ray_sample(compound_of("far_apart"), RAD, w)
    assert np.array_equal(bits(got), bits(reading("far_apart", R.SURFACE)[0]))


def test_cpp_mirror_compound_sampling_example(hip_lib):
    """examples/compound_sampling3.cpp: include/salva_hip.hpp's three overloads for a `salva::Compound` — a boundary sampled from the
    five-slab box, fluid poured in from the volume sample of a second compound, the surface sample read back.  The fluid ends in the
    box, on its floor."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "compound_sampling3"], check=True, capture_output=True)
    out = subprocess.run([os.path.join(ROOT, "examples", "compound_sampling3"), "200"], check=True, capture_output=True, text=True, timeout=300).stdout
    print(out)
    rows = [re.search(r"step (\d+): (\d+) fluid particles poured, (\d+) in the box, lowest y ([0-9.e+-]+) \(floor top ([0-9.e+-]+)\); (\d+) boundary samples "
                      r"\((\d+) sampled to the host\)", l) for l in out.strip().splitlines()]
    assert len(rows) == 4 and all(rows), out
    last = rows[-1]
    assert int(last.group(2)) > 300 and int(last.group(3)) == int(last.group(2)), out      # nothing leaks through the sampled walls
    assert float(last.group(4)) > float(last.group(5)) - 0.025, out                        # ... or through the floor
    # the boundary holds the surface sample: the slabs are thinner than a spacing, so a slab's two faces share a lattice layer — one
    # point per s^2 of the four walls alone (4 x 0.8 x 0.5 / 0.05^2) is 640
    assert int(last.group(6)) == int(last.group(7)) >= 640, out


def test_decomposed_world_refuses_the_editing_calls(hip_lib):
    r = 0.025
    pos = scenes.cube_fluid_positions(16, 6, 6, r)
    w = LiquidWorld(DFSPHSolver(), r, 2.0)
    w.add_fluid(Fluid(pos, r, 1000.0))
    comm = dist.Comm.loopback(1)[0]
    cx = dist.cell_x(pos, w.h())
    w.set_domain(comm, int(cx.min()), int(cx.max()), 0)
    w.step(DT, G)
    h = compound_of("far_apart").handle(w)
    t, q = np.zeros(3, F), F([0, 0, 0, 1])
    assert w._L.salva_hip_add_particles_sampled_compound(w._h, 0, h, t.ctypes.data_as(FP), q.ctypes.data_as(FP), 1, None) == _lib.E_INVALID
    assert "salva_hip_add_particles" in last_error(w)
    assert w._L.salva_hip_set_boundary_sampling_from_compound(w._h, 0, h, 1, 0xFFFFFFFF) == _lib.E_INVALID
    assert "salva_hip_add_particles" in last_error(w)
    w.step(DT, G)
    gid, p, _, _ = w.owned()
    assert len(gid) == len(pos) and np.isfinite(p).all()
    del w
    comm.destroy()
