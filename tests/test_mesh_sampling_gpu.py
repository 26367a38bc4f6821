"""The ray sampler on a triangle mesh (salva_amd/csrc/sample.hip k_sample_mesh_mark) against the host arm driven by
the numpy cast and against the pure-numpy reading (tests/mesh_reading.py), bit for bit; the two ways to use the samples without a
host round trip; the error cases."""
import ctypes as C
import functools

import numpy as np
import pytest

import mesh_fixtures as X
import mesh_reading as M
import sampling_reading as R
from salva_amd import Boundary, DFSPHSolver, Fluid, LiquidWorld, _lib, sampling
from salva_amd.coupling import ColliderCouplingSet, StaticSampling

pytestmark = pytest.mark.gpu

F = np.float32
RAD = 0.0125
FP = C.POINTER(C.c_float)
UP = C.POINTER(C.c_uint32)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@functools.lru_cache(maxsize=None)
def reading(name, mode):
    fixture, rad = X.ALL[name]
    v, t, _ = fixture()
    q, pos, N = M.sample_mesh(v, t, rad, mode)
    pos.setflags(write=False)
    return pos, N


@pytest.fixture(scope="module")
def world(hip_lib):
    return LiquidWorld(DFSPHSolver(), RAD, 2.0)


def mesh_of(fixture):
    v, t, oriented = fixture()
    return sampling.Mesh(v, t, oriented=oriented)


@pytest.mark.parametrize("mode", [R.SURFACE, R.VOLUME])
@pytest.mark.parametrize("name", list(X.ALL))
def test_device_equals_host_arm_and_reading(world, name, mode):
    fixture, rad = X.ALL[name]
    v, t, _ = fixture()
    ref, N = reading(name, mode)
    assert max(N) <= 40
    got = sampling._sample(mesh_of(fixture), rad, mode, world)
    host = sampling._sample(sampling.HostRayShape(lambda: M.mesh_aabb(v), lambda origins, axis: M.mesh_cast(v, t, origins, axis)), rad, mode, world)
    print(name, mode, "lattice", N, "reading", len(ref), "host arm", len(host), "device", len(got))
    assert len(ref) > 0
    assert len(got) == len(host) and np.array_equal(bits(got), bits(host))
    assert len(got) == len(ref) and np.array_equal(bits(got), bits(ref))


def test_heightfield_entry_point_equals_the_triangles(world):
    heights = X._heights(5, 11)
    ref, _ = reading("heightfield5", R.SURFACE)
    got = sampling._sample(sampling.Mesh.heightfield(heights, (1.0, 0.3, 1.2)), X.ALL["heightfield5"][1], R.SURFACE, world)
    assert len(got) == len(ref) and np.array_equal(bits(got), bits(ref))


def test_cube_volume_equals_the_cuboid_on_the_device(world):
    got = sampling._sample(mesh_of(X.cube), 0.0625, R.VOLUME, world)
    cub = sampling._sample(("cuboid", (0.5, 0.5, 0.5)), 0.0625, R.VOLUME, world)
    assert len(got) == len(cub) > 0 and np.array_equal(bits(got), bits(cub))


def test_fluid_and_boundary_from_mesh_equal_uploaded_samples(hip_lib):
    """add_particles_from_shape(mesh) and StaticSampling.from_shape(mesh) leave on the device what uploading the reading's points by
    hand leaves there (identity pose: the posed emit is the analytic shapes', tested with them)."""
    v, t, _ = X.tetrahedron()
    _, vol, _ = M.sample_mesh(v, t, RAD, R.VOLUME)
    _, surf, _ = M.sample_mesh(v, t, RAD, R.SURFACE)
    vel = F([0.1, -0.2, 0.3])
    res = []
    for from_mesh in (True, False):
        w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
        f = w.add_fluid(Fluid(F([[5.0, 5.0, 5.0]]), RAD, 1000.0))  # (one particle far away: a fluid that exists on the device)
        b = w.add_boundary(Boundary([]))
        cs = ColliderCouplingSet()
        mesh = mesh_of(X.tetrahedron)
        cs.register_coupling(b, "tet", None, StaticSampling.from_shape(mesh) if from_mesh else StaticSampling(surf))
        w.sync_to_device()
        if from_mesh:
            assert f.add_particles_from_shape(mesh, velocity=vel) == len(vol)
        else:
            f.add_particles(vol, np.tile(vel, (len(vol), 1)))
            w.sync_to_device()
        cs.update_boundaries(w)
        assert b.num_particles() == len(surf)
        bp, bv = w._boundary_particles(b)
        res.append((np.array(f.positions)[1:], np.array(f.velocities)[1:], np.array(bp), np.array(bv)))
    assert len(res[0][0]) == len(vol) > 0 and len(res[0][2]) == len(surf) > 0
    for a, b_ in zip(res[0], res[1]):
        assert np.array_equal(bits(a), bits(b_))
    assert np.array_equal(bits(res[0][0]), bits(vol)) and np.array_equal(bits(res[0][2]), bits(surf))


def test_mesh_errors(world):
    w = world
    v, t, _ = X.cube()
    h = C.c_uint32(12345)

    def create(vv, tt, flags=0):
        vv, tt = np.ascontiguousarray(vv, F), np.ascontiguousarray(tt, np.uint32)
        return w._L.salva_hip_create_mesh(w._h, vv.ctypes.data_as(FP), len(vv), tt.ctypes.data_as(UP), len(tt), flags, C.byref(h))

    bad = t.copy()
    bad[3, 1] = 8
    assert create(v, bad) == _lib.E_INVALID                      # an index past the vertices
    assert create(v, t[:0]) == _lib.E_INVALID                    # no triangles
    nan = v.copy()
    nan[2, 1] = np.nan
    assert create(nan, t) == _lib.E_INVALID                      # a non-finite vertex
    hf = np.zeros((1, 5), F)
    scale = F([1, 1, 1])
    assert w._L.salva_hip_create_heightfield(w._h, hf.ctypes.data_as(FP), 1, 5, scale.ctypes.data_as(FP), C.byref(h)) == _lib.E_INVALID
    assert w._L.salva_hip_create_heightfield(w._h, hf.ctypes.data_as(FP), 5, 1, scale.ctypes.data_as(FP), C.byref(h)) == _lib.E_INVALID
    assert w._L.salva_hip_sample_mesh(w._h, 9999, 0.05, 0, 0, None) == _lib.E_INVALID
    # a mesh in use cannot be destroyed; clearing the sampling releases it
    assert create(v, t, _lib.MESH_ORIENTED) == _lib.OK
    w2 = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    w2.add_fluid(Fluid(np.zeros((1, 3), F), RAD, 1000.0))
    b = w2.add_boundary(Boundary([]))
    w2.sync_to_device()
    mesh = mesh_of(X.cube)
    mh = mesh.handle(w2)
    _lib.check(w2._L.salva_hip_set_boundary_dynamic_sampling_mesh(w2._h, b._slot, mh, 1, 0xFFFFFFFF))
    assert w2._L.salva_hip_destroy_mesh(w2._h, mh) == _lib.E_INVALID
    _lib.check(w2._L.salva_hip_clear_boundary_sampling(w2._h, b._slot))
    assert w2._L.salva_hip_destroy_mesh(w2._h, mh) == _lib.OK
    assert w2._L.salva_hip_destroy_mesh(w2._h, mh) == _lib.E_INVALID  # gone
    # a ray through 40 slabs is hit 80 times
    sv, st, _ = X.slabs()
    with pytest.raises(_lib.SalvaHipError) as e:
        sampling._sample(sampling.Mesh(sv, st, oriented=True), 0.05, R.SURFACE, w)
    assert e.value.code == _lib.E_CAPACITY
    # ... and a stack the bound admits is sampled like any mesh
    sv, st, _ = X.slabs(20)
    got = sampling._sample(sampling.Mesh(sv, st, oriented=True), 0.05, R.SURFACE, w)
    _, ref, _ = M.sample_mesh(sv, st, 0.05, R.SURFACE)
    assert len(got) == len(ref) > 0 and np.array_equal(bits(got), bits(ref))
