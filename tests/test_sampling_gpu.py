"""The ray sampler on the device (salva_amd/csrc/sample.hip) against tests/sampling_reading.py — bit for bit: every
operation involved is a correctly rounded f32 operation on both sides — and the three ways to use it without a host round trip."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import sampling_reading as R
from salva_amd import Boundary, DFSPHSolver, Fluid, LiquidWorld, NonPressureForce, _lib, dist, sampling, scenes
from salva_amd.coupling import ColliderCouplingSet, RigidBody, StaticSampling, make_shape

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
RAD = 0.0125
DT = 1.0 / 200.0
G = (0.0, -9.81, 0.0)
FP = C.POINTER(C.c_float)
# a 40 x 40 x 70 lattice: z rows of three words that end mid-word, 3 500 words = more than one scan block; dyadic numbers, so that the
# faces' half-way ties round exactly (tests/test_sampling_cpu.py::test_cuboid_volume_is_the_full_block)
EDGE_CUBOID, EDGE_RAD = ("cuboid", (2.359375, 2.359375, 4.234375)), 0.0625


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@functools.lru_cache(maxsize=None)
def reading(shape, rad, mode):
    q, pos, N = R.sample(shape, rad, mode)
    pos.setflags(write=False)
    return q, pos, N


@functools.lru_cache(maxsize=None)
def thin_ball():
    return ("ball", R.find_thin_chord_ball())


@pytest.fixture(scope="module")
def world(hip_lib):
    return LiquidWorld(DFSPHSolver(), RAD, 2.0)


def raw_sample(w, shape, rad, mode, capacity, out):
    s = make_shape(shape)
    return int(w._L.salva_hip_sample_shape(w._h, C.byref(s), rad, mode, capacity, out.ctypes.data_as(FP) if out is not None else None))


def last_error(w):
    return w._L.salva_hip_last_error().decode()


# ---------------------------------------------------------------------------------------------- 1. device against the reading
SHAPES = [("ball", 0.15), ("capsule", 0.2, 0.1), ("cylinder", 0.15, 0.12), "thin"]


@pytest.mark.parametrize("mode", [R.SURFACE, R.VOLUME])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s if isinstance(s, str) else s[0])
def test_device_equals_reading(world, shape, mode):
    shape = thin_ball() if shape == "thin" else shape
    q, ref, N = reading(shape, RAD, mode)
    got = sampling._sample(shape, RAD, mode, world)
    print(shape, mode, "lattice", N, "reading", len(ref), "device", len(got))
    assert len(got) == len(ref) and len(ref) > 0
    assert np.array_equal(bits(got), bits(ref))
    assert [tuple(r) for r in q] == sorted(tuple(r) for r in q)  # lexicographic, x slowest


@pytest.mark.parametrize("mode", [R.SURFACE, R.VOLUME])
def test_basic3_wall_cuboid_equals_reading(world, mode):
    shape = ("cuboid", (0.2, 0.7, 2.5))
    _, ref, _ = reading(shape, 0.05, mode)
    got = sampling._sample(shape, 0.05, mode, world)
    assert len(got) == len(ref) and np.array_equal(bits(got), bits(ref))
    if mode == R.SURFACE:
        assert len(got) == 1648 and np.array_equal(bits(got), bits(scenes.cuboid_surface_ray_sample([0.2, 0.7, 2.5], 0.05)))


# ---------------------------------------------------------------------------------------------- 2. word and scan edges
@pytest.mark.parametrize("mode", [R.SURFACE, R.VOLUME])
def test_rows_across_words_and_scan_blocks(world, mode):
    _, ref, N = reading(EDGE_CUBOID, EDGE_RAD, mode)
    assert N == [40, 40, 70]
    got = sampling._sample(EDGE_CUBOID, EDGE_RAD, mode, world)
    assert len(got) == len(ref) and np.array_equal(bits(got), bits(ref))
    if mode == R.VOLUME:
        assert len(got) == 38 * 38 * 68


# ---------------------------------------------------------------------------------------------- 3. capacity convention
def test_capacity_one_short_leaves_the_buffer_alone(world):
    shape = ("ball", 0.15)
    _, ref, _ = reading(shape, RAD, R.SURFACE)
    n = len(ref)
    out = np.full((n, 3), 123.25, F)
    assert raw_sample(world, shape, RAD, R.SURFACE, n - 1, out) == n
    assert (out == F(123.25)).all()
    assert raw_sample(world, shape, RAD, R.SURFACE, 0, None) == n
    assert raw_sample(world, shape, RAD, R.SURFACE, n, out) == n
    assert np.array_equal(bits(out), bits(ref))


# ---------------------------------------------------------------------------------------------- 4. boundary from shape
FLOOR = ("cuboid", (0.2, 0.03, 0.2))
BLOCK = ("cuboid", (0.06, 0.05, 0.07))


def moving_body():
    return RigidBody(translation=np.array([0.02, -0.01, 0.03], F), rotation=scenes.quat_from_scaled_axis([0.1, 0.3, -0.2]),
                     linvel=np.array([0.1, 0.0, -0.05], F), angvel=np.array([0.0, 0.4, 0.1], F), local_com=np.array([0.01, 0.0, 0.0], F),
                     mass=50.0, dynamic=True)


def coupled_world(static_sampling, fluid_points):
    w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    f = w.add_fluid(Fluid(fluid_points, RAD, 1000.0))
    b = w.add_boundary(Boundary([]))
    cs = ColliderCouplingSet()
    body = moving_body()
    cs.register_coupling(b, "floor", body, static_sampling)
    return w, f, b, cs, body


def test_boundary_from_shape_equals_uploaded_samples(hip_lib):
    _, floor_pts, _ = reading(FLOOR, RAD, R.SURFACE)
    _, block_pts, _ = reading(BLOCK, RAD, R.VOLUME)
    fluid = (block_pts + np.array([0.0, 0.12, 0.0], F)).astype(F)
    res = []
    for ss in (StaticSampling.from_shape(FLOOR), StaticSampling(floor_pts)):
        w, f, b, cs, body = coupled_world(ss, fluid)
        w.sync_to_device()
        cs.update_boundaries(w)
        assert b.num_particles() == len(floor_pts)
        pos, vel = w._boundary_particles(b)
        wrenches = []
        for _ in range(5):
            w.sync_to_device()
            cs.update_boundaries(w)
            w.step(DT, G)
            fo, to = np.zeros(3, F), np.zeros(3, F)
            com = body.center_of_mass()
            _lib.check(w._L.salva_hip_get_boundary_wrench(w._h, b._slot, com.ctypes.data_as(FP), fo.ctypes.data_as(FP), to.ctypes.data_as(FP)))
            wrenches.append((fo, to))
        res.append((pos, vel, wrenches, f.positions.copy()))
    (p0, v0, w0, f0), (p1, v1, w1, f1) = res
    assert np.array_equal(bits(p0), bits(p1)) and np.array_equal(bits(v0), bits(v1))
    assert np.abs(v0).max() > 0  # the pose moves
    for (fa, ta), (fb, tb) in zip(w0, w1):
        assert np.array_equal(bits(fa), bits(fb)) and np.array_equal(bits(ta), bits(tb))
    assert np.abs(w0[-1][0]).max() > 0  # the fluid has reached the floor: the wrench compares something
    assert np.array_equal(bits(f0), bits(f1))


# ---------------------------------------------------------------------------------------------- 5. fluid from shape
def test_fluid_from_shape_identity_rotation(hip_lib):
    _, pts, _ = reading(BLOCK, RAD, R.VOLUME)
    t, v = np.array([0.3, -0.2, 0.15], F), np.array([0.25, -1.0, 0.5], F)
    w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    f = w.add_fluid(Fluid([], RAD, 1000.0))
    assert f.add_particles_from_shape(BLOCK, t, (0, 0, 0, 1), R.VOLUME, v) == len(pts)
    assert f.num_particles() == len(pts)
    assert np.array_equal(bits(f.positions), bits((pts + t).astype(F)))
    assert np.array_equal(bits(f.velocities), bits(np.tile(v, (len(pts), 1))))
    # surface mode and no velocity
    _, spts, _ = reading(BLOCK, RAD, R.SURFACE)
    assert f.add_particles_from_shape(BLOCK, t, (0, 0, 0, 1), R.SURFACE) == len(spts)
    assert np.array_equal(bits(f.positions[len(pts):]), bits((spts + t).astype(F))) and not f.velocities[len(pts):].any()
    assert np.array_equal(bits(f.positions[:len(pts)]), bits((pts + t).astype(F)))


def test_fluid_from_shape_rotated_pose_equals_boundary_pose(hip_lib):
    shape = ("capsule", 0.05, 0.04)
    _, pts, _ = reading(shape, RAD, R.VOLUME)
    body = moving_body()
    w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    f = w.add_fluid(Fluid([], RAD, 1000.0))
    b = w.add_boundary(Boundary([]))
    cs = ColliderCouplingSet()
    cs.register_coupling(b, "c", body, StaticSampling(pts))
    w.sync_to_device()
    cs.update_boundaries(w)
    posed = w._boundary_particles(b)[0]
    assert f.add_particles_from_shape(shape, body.translation, body.rotation, R.VOLUME) == len(pts)
    assert np.array_equal(bits(f.positions), bits(posed))
    assert np.abs(posed - pts).max() > 1e-3


def test_sampled_world_steps_like_uploaded_world(hip_lib):
    _, floor_pts, _ = reading(FLOOR, RAD, R.SURFACE)
    _, block_pts, _ = reading(BLOCK, RAD, R.VOLUME)
    t = np.array([0.0, 0.1, 0.0], F)
    runs = []
    for device in (True, False):
        w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
        f = w.add_fluid(Fluid([], RAD, 1000.0))
        b = w.add_boundary(Boundary([]))
        cs = ColliderCouplingSet()
        cs.register_coupling(b, "floor", None, StaticSampling.from_shape(FLOOR) if device else StaticSampling(floor_pts))
        if device:
            f.add_particles_from_shape(BLOCK, t, (0, 0, 0, 1), R.VOLUME)
        else:
            f.add_particles((block_pts + t).astype(F))
        iters = []
        for _ in range(5):
            st = w.step_with_coupling(DT, G, cs)
            iters.append((st.n_divergence_iters, st.n_pressure_iters))
        runs.append((f.positions.copy(), f.velocities.copy(), iters, w._boundary_particles(b)[0]))
    a, c = runs
    assert a[2] == c[2]
    assert np.array_equal(bits(a[0]), bits(c[0])) and np.array_equal(bits(a[1]), bits(c[1])) and np.array_equal(bits(a[3]), bits(c[3]))
    assert len(a[0]) == len(block_pts) and np.isfinite(a[0]).all()


# ---------------------------------------------------------------------------------------------- 6. emitter
def test_emitter_adds_sampled_balls_to_a_living_fluid(hip_lib):
    ball = ("ball", 0.04)
    _, ball_pts, _ = reading(ball, RAD, R.VOLUME)
    _, block_pts, _ = reading(BLOCK, RAD, R.VOLUME)
    _, floor_pts, _ = reading(FLOOR, RAD, R.SURFACE)
    v = np.array([0.0, -1.0, 0.0], F)
    runs = []
    for device in (True, False):
        w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
        f = w.add_fluid(Fluid((block_pts + np.array([0.0, 0.1, 0.0], F)).astype(F), RAD, 1000.0))
        w.add_boundary(Boundary(floor_pts))
        counts, step = [], 0
        for k in range(4):
            for _ in range(3):
                w.step(DT, G)
                step += 1
            before = f.positions.copy()
            t = np.array([0.01 * k, 0.3, -0.01 * k], F)
            if device:
                assert f.add_particles_from_shape(ball, t, (0, 0, 0, 1), R.VOLUME, v) == len(ball_pts)
            else:
                f.add_particles((ball_pts + t).astype(F), np.tile(v, (len(ball_pts), 1)))
            counts.append(f.num_particles())
            after = f.positions
            assert np.array_equal(bits(after[:len(before)]), bits(before))  # earlier particles keep their indices
            assert np.array_equal(bits(after[len(before):]), bits((ball_pts + t).astype(F)))
        w.step(DT, G)
        runs.append((counts, f.positions.copy(), f.velocities.copy()))
    n0 = len(block_pts)
    assert runs[0][0] == runs[1][0] == [n0 + (k + 1) * len(ball_pts) for k in range(4)]
    assert np.array_equal(bits(runs[0][1]), bits(runs[1][1])) and np.array_equal(bits(runs[0][2]), bits(runs[1][2]))


# ---------------------------------------------------------------------------------------------- 7. host arm
def intervals_cast(intervals_of):
    """`cast_local_ray(ray, MAX, solid = false)` from interval lists: the first interval boundary ahead of the origin."""
    hits = {}

    def cast(origins, axis):
        j, k = (axis + 1) % 3, (axis + 2) % 3
        toi = np.full(len(origins), -1.0, F)
        for r, o in enumerate(origins):
            for a, b in intervals_of(axis, o[j], o[k]):
                if o[axis] <= a:
                    toi[r] = F(a - o[axis])
                elif o[axis] < b:
                    toi[r] = F(b - o[axis])
                else:
                    continue
                key = (axis, float(o[j]), float(o[k]))
                hits[key] = hits.get(key, 0) + 1
                break
        return toi

    return cast, hits


def test_host_arm_ball_equals_device_ball(world):
    Rb = F(0.15)

    def intervals_of(i, cj, ck):
        d2 = F(F(Rb * Rb) - F(F(cj * cj) + F(ck * ck)))
        if not d2 > 0:
            return []
        h = F(np.sqrt(d2))
        return [(F(-h), h)]

    for mode in (R.SURFACE, R.VOLUME):
        cast, _ = intervals_cast(intervals_of)
        shape = sampling.HostRayShape(lambda: ((-Rb, -Rb, -Rb), (Rb, Rb, Rb)), cast)
        got = sampling._sample(shape, RAD, mode, world)
        dev = sampling._sample(("ball", 0.15), RAD, mode, world)
        assert len(got) == len(dev) > 0 and np.array_equal(bits(got), bits(dev))


def test_host_arm_concave_two_balls(world):
    mins, maxs, intervals_of = R.two_balls_intervals(0.1, 0.15)
    for mode in (R.SURFACE, R.VOLUME):
        cast, hits = intervals_cast(intervals_of)
        shape = sampling.HostRayShape(lambda: (mins, maxs), cast)
        got = sampling._sample(shape, RAD, mode, world)
        _, ref, _ = R.sample_intervals(mins, maxs, RAD, mode, intervals_of)
        assert len(got) == len(ref) > 0 and np.array_equal(bits(got), bits(ref))
        through_both = [n for (axis, cj, ck), n in hits.items() if axis == 0 and len(intervals_of(0, F(cj), F(ck))) == 2]
        assert through_both and set(through_both) == {4}  # four impacts per x-ray through both balls
        assert max(hits.values()) == 4


def test_host_arm_gives_up_after_64_rounds(world):
    calls = []

    def cast(origins, axis):
        calls.append(len(origins))
        return np.full(len(origins), 0.01, F)

    shape = sampling.HostRayShape(lambda: ((-0.02, -0.02, -0.02), (0.02, 0.02, 0.02)), cast)
    with pytest.raises(_lib.SalvaHipError) as e:
        sampling._sample(shape, RAD, R.SURFACE, world)
    assert e.value.code == _lib.E_INVALID and "64 rounds" in str(e.value)
    assert len(calls) == 64
    assert len(sampling.shape_surface_ray_sample(("ball", 0.15), RAD, world)) == len(reading(("ball", 0.15), RAD, R.SURFACE)[1])


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_lattice_over_2_to_32_is_a_capacity_error(world):
    assert raw_sample(world, ("cuboid", (100.0, 100.0, 100.0)), RAD, R.VOLUME, 0, None) == _lib.E_CAPACITY
    assert "2^32" in last_error(world)
    s = make_shape(("cuboid", (100.0, 100.0, 100.0)))
    w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    f = w.add_fluid(Fluid(scenes.cube_fluid_positions(4, 4, 4, RAD), RAD, 1000.0))
    w.sync_to_device()
    t, q = np.zeros(3, F), np.array([0, 0, 0, 1], F)
    assert w._L.salva_hip_add_particles_sampled(w._h, 0, C.byref(s), t.ctypes.data_as(FP), q.ctypes.data_as(FP), 1, None) == _lib.E_CAPACITY
    assert w._L.salva_hip_set_boundary_sampling_from_shape(w._h, 0, C.byref(s), 1, 0xFFFFFFFF) == _lib.E_CAPACITY
    w.step(DT, G)
    assert f.num_particles() == 64 and np.isfinite(f.positions).all()


def test_decomposed_world_refuses_the_mutating_calls(hip_lib):
    r = 0.025
    pos = scenes.cube_fluid_positions(16, 6, 6, r)
    w = LiquidWorld(DFSPHSolver(), r, 2.0)
    f = w.add_fluid(Fluid(pos, r, 1000.0))
    comm = dist.Comm.loopback(1)[0]
    cx = dist.cell_x(pos, w.h())
    w.set_domain(comm, int(cx.min()), int(cx.max()), 0)
    w.step(DT, G)
    s = make_shape(("ball", 0.1))
    t, q = np.zeros(3, F), np.array([0, 0, 0, 1], F)
    assert w._L.salva_hip_add_particles_sampled(w._h, 0, C.byref(s), t.ctypes.data_as(FP), q.ctypes.data_as(FP), 1, None) == _lib.E_INVALID
    assert "salva_hip_add_particles" in last_error(w)
    assert w._L.salva_hip_set_boundary_sampling_from_shape(w._h, 0, C.byref(s), 1, 0xFFFFFFFF) == _lib.E_INVALID
    assert "salva_hip_add_particles" in last_error(w)
    got = sampling.shape_surface_ray_sample(("ball", 0.15), RAD, w)  # sampling itself works there
    assert np.array_equal(bits(got), bits(reading(("ball", 0.15), RAD, R.SURFACE)[1]))
    w.step(DT, G)
    gid, p, v, _ = w.owned()
    assert len(gid) == len(pos) and np.isfinite(p).all()
    del w
    comm.destroy()


class CallsTheSampler(NonPressureForce):
    def __init__(self):
        self.codes = None

    def solve(self, timestep, kernel_radius, ff, fb, fluid, boundaries, densities):
        w = self.world
        s = make_shape(("ball", 0.05))
        t, q = np.zeros(3, F), np.array([0, 0, 0, 1], F)
        out = np.zeros((4, 3), F)
        hs = sampling.HostRayShape(lambda: ((-1, -1, -1), (1, 1, 1)), lambda o, a: np.full(len(o), -1.0, F))
        self.codes = [
            int(w._L.salva_hip_sample_shape(w._h, C.byref(s), RAD, 0, 0, out.ctypes.data_as(FP))),
            int(w._L.salva_hip_sample_host_shape(w._h, C.byref(hs.shape), RAD, 0, 0, out.ctypes.data_as(FP))),
            int(w._L.salva_hip_add_particles_sampled(w._h, 0, C.byref(s), t.ctypes.data_as(FP), q.ctypes.data_as(FP), 1, None)),
            int(w._L.salva_hip_set_boundary_sampling_from_shape(w._h, 0, C.byref(s), 1, 0xFFFFFFFF)),
        ]
        self.message = last_error(w)


def test_calls_inside_a_force_callback_are_refused(hip_lib):
    w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    f = Fluid(scenes.cube_fluid_positions(5, 5, 5, RAD), RAD, 1000.0)
    force = CallsTheSampler()
    force.world = w
    f.nonpressure_forces.append(force)
    w.add_fluid(f)
    w.step(DT, G)
    assert force.codes == [_lib.E_INVALID] * 4 and "force callback" in force.message
    w.step(DT, G)
    assert f.num_particles() == 125 and np.isfinite(f.positions).all() and w._L.salva_hip_num_boundaries(w._h) == 0


# ---------------------------------------------------------------------------------------------- the mirrors
def test_python_mirror_calls(world):
    got = sampling.shape_volume_ray_sample(("cylinder", 0.15, 0.12), RAD, world)
    assert np.array_equal(bits(got), bits(reading(("cylinder", 0.15, 0.12), RAD, R.VOLUME)[1]))
    own = sampling.shape_surface_ray_sample(("ball", 0.15), RAD)  # a world of its own
    assert np.array_equal(bits(own), bits(scenes.ball_surface_ray_sample(0.15, RAD)))


def test_cpp_mirror_calls(hip_lib, tmp_path):
    exe, dump = tmp_path / "sampling_mirror", tmp_path / "dump.bin"
    lib = os.path.join(ROOT, "salva_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "sampling_mirror.cpp"),
                           f"-L{lib}", "-lsalva_hip", f"-Wl,-rpath,{lib}"])
    r = subprocess.run([str(exe), str(dump)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    raw = dump.read_bytes()
    arrays, o = [], 0
    while o < len(raw):
        n = int(np.frombuffer(raw, np.uint64, 1, o)[0])
        arrays.append(np.frombuffer(raw, F, 3 * n, o + 8).reshape(n, 3))
        o += 8 + 12 * n
    assert len(arrays) == 5
    _, block_pts, _ = reading(BLOCK, RAD, R.VOLUME)
    assert np.array_equal(bits(arrays[0]), bits(reading(("ball", 0.15), RAD, R.SURFACE)[1]))
    assert np.array_equal(bits(arrays[1]), bits(reading(("capsule", 0.2, 0.1), RAD, R.VOLUME)[1]))
    assert np.array_equal(bits(arrays[2]), bits((block_pts + np.array([0.01, 0.12, -0.02], F)).astype(F)))
    assert np.array_equal(bits(arrays[3]), bits(reading(FLOOR, RAD, R.SURFACE)[1]))
    # the same two steps through the Python mirror
    w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    f = w.add_fluid(Fluid([], RAD, 1000.0))
    b = w.add_boundary(Boundary([]))
    cs = ColliderCouplingSet()
    cs.register_coupling(b, "floor", None, StaticSampling.from_shape(FLOOR))
    f.add_particles_from_shape(BLOCK, (0.01, 0.12, -0.02), (0, 0, 0, 1), R.VOLUME, (0.0, -0.5, 0.0))
    w.sync_to_device()
    cs.update_boundaries(w)
    for _ in range(2):
        w.step(DT, G)
    assert np.array_equal(bits(arrays[4]), bits(f.positions))
