"""Ray casts at the fluid (salva_hip_cast_rays / _cast_rays_camera) on the device against the brute-force reading
tests/fluid_ray_reading.py: t, fluid, index and normal bit for bit with no ray left out, the thickness within
(n + 16) 2^-24 sum |chord| (a sum in another order)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fluid_ray_child as rc
import fluid_ray_reading as rr
from salva_amd import _lib

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
F = np.float32
H = rr.H32
R0 = rr.R_PARTICLE


def compare(got, ref, what=""):
    """everything a call returned against the reading"""
    m = len(ref["t"])
    if "t" in got:
        for k in ("t", "fluid", "index"):
            a, b = np.ascontiguousarray(got[k]).reshape(-1), ref[k]
            bad = np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0]
            assert not len(bad), (what, k, len(bad), bad[:5], a[bad[:5]], b[bad[:5]])
    if "normal" in got:
        a, b = np.ascontiguousarray(got["normal"]).reshape(m, 3), ref["normal"]
        bad = np.nonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))[0]
        assert not len(bad), (what, "normal", len(bad), bad[:5], a[bad[:5]], b[bad[:5]])
    if "thickness" in got:
        a = np.ascontiguousarray(got["thickness"]).reshape(-1).astype(np.float64)
        err, tol = np.abs(a - ref["thickness"]), rr.thickness_tolerance(ref)
        assert (err <= tol).all(), (what, "thickness", float((err - tol).max()))
        assert (a[ref["A"] == 0] == 0).all()


def last_error():
    return _lib.lib().salva_hip_last_error().decode()


@pytest.fixture(scope="module")
def case():
    return rr.standard_case()


@pytest.fixture(scope="module")
def world(hip_lib, case):
    return rr.make_world(case["x"], case["slots"])


# ------------------------------------------------------------------------------------------------ the standard case
@pytest.mark.parametrize("which", [0, 1])
def test_standard_rays(world, case, which):
    w, _ = world
    R = case["radii"][which]
    ref = rr.cast(case["origins"], case["directions"], case["x"], case["slots"], R)
    assert (ref["row"] >= 0).sum() > 1000 and (ref["row"] < 0).sum() > 100 and ref["n"].max() > 5
    assert len(np.unique(ref["fluid"])) == 3
    got = w.cast_rays(case["origins"], case["directions"], radius=R, normals=True, thickness=True)
    compare(got, ref, "rays")
    again = w.cast_rays(case["origins"], case["directions"], radius=R, normals=True, thickness=True)
    for k in got:
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), k  # (one lane per ray, a fixed walk: the thickness too)
    # first hit only and thickness only, against the combined call
    first = w.cast_rays(case["origins"], case["directions"], radius=R, normals=True)
    assert set(first) == {"t", "fluid", "index", "normal"}
    for k in first:
        assert np.array_equal(first[k].view(np.uint32), got[k].view(np.uint32)), k
    plain = w.cast_rays(case["origins"], case["directions"], radius=R)
    assert set(plain) == {"t", "fluid", "index"} and all(np.array_equal(plain[k], got[k]) for k in plain)
    only = w.cast_rays(case["origins"], case["directions"], radius=R, thickness=True, hits=False)
    assert set(only) == {"thickness"} and np.array_equal(only["thickness"].view(np.uint32), got["thickness"].view(np.uint32))


def test_standard_camera(world, case):
    w, _ = world
    cam = case["camera"]
    o, d = rr.camera_rays(cam)
    ref = rr.cast(o, d, case["x"], case["slots"], R0)
    assert (ref["row"] >= 0).sum() > 500 and (ref["row"] < 0).sum() > 100
    got = w.cast_camera(cam, normals=True, thickness=True)
    assert got["t"].shape == (48, 64) and got["normal"].shape == (48, 64, 3)
    compare(got, ref, "camera")
    # the same rays from a list
    lst = w.cast_rays(o, d, normals=True, thickness=True)
    for k in lst:
        assert np.array_equal(lst[k].reshape(-1).view(np.uint32), got[k].reshape(-1).view(np.uint32)), k
    # a camera whose width and height are no multiples of the tile
    odd = dict(cam, width=13, height=9)
    oo, dd = rr.camera_rays(odd)
    compare(w.cast_camera(odd, normals=True, thickness=True), rr.cast(oo, dd, case["x"], case["slots"], R0), "odd camera")


# ------------------------------------------------------------------------------------------------ where the walk can go wrong
def small_scene():
    """A jittered 6 x 5 x 4 block at 2 r (fluid 0) and, in fluid 1: particles exactly on cell boundaries (multiples of h in all three
    coordinates, and in one), two at the position of fluid 0's row 7 and of each other (the tie), and 500 in one cell."""
    rng = np.random.default_rng(3)
    r = R0
    ix, iy, iz = np.meshgrid(np.arange(6), np.arange(5), np.arange(4), indexing="ij")
    a = (np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1) * (2.0 * r) + 0.013 + rng.uniform(-0.3 * r, 0.3 * r, (120, 3))).astype(F)
    on = np.array([[F(1) * H, F(2) * H, F(1) * H], [F(2) * H, F(0.37), F(0.11)], [F(0.21), F(1) * H, F(0.17)], [F(3) * H, F(2) * H, F(0.05)]], F)
    crowd = (np.array([4.1, 1.1, 2.1]) * float(H) + rng.uniform(0.0, 0.8 * float(H), (500, 3))).astype(F)
    assert (np.floor(crowd / H) == np.floor(crowd[0] / H)).all()
    b = np.concatenate([on, a[7:8], a[7:8], crowd]).astype(F)
    x = np.concatenate([a, b])
    return x, np.concatenate([np.zeros(len(a), np.uint32), np.ones(len(b), np.uint32)])


@pytest.fixture(scope="module")
def small(hip_lib):
    x, slots = small_scene()
    w, fluids = rr.make_world(x, slots)
    return w, fluids, x, slots


def through(x, rng, m):
    """m rays from outside aimed at random particles, with a small offset"""
    tgt = x[rng.integers(0, len(x), m)].astype(np.float64) + rng.uniform(-0.02, 0.02, (m, 3))
    o = tgt + rng.normal(size=(m, 3)) * 0.4 + np.sign(rng.normal(size=(m, 3))) * 0.3
    return o.astype(F), (tgt - o).astype(F)


def edge_rays(name, x):
    rng = np.random.default_rng(17)
    lo, hi = x.min(axis=0).astype(np.float64), x.max(axis=0).astype(np.float64)
    if name == "axes":  # two components of d exactly 0, both senses, origins outside and inside
        o, d = [], []
        for k in range(3):
            for sgn in (1.0, -1.0):
                p = rng.uniform(lo - 0.05, hi + 0.05, (40, 3))
                p[:20, k] = lo[k] - 0.3 if sgn > 0 else hi[k] + 0.3
                e = np.zeros((40, 3))
                e[:, k] = sgn * rng.uniform(0.5, 2.0, 40)
                o.append(p), d.append(e)
        return np.concatenate(o).astype(F), np.concatenate(d).astype(F)
    if name == "faces":  # rays lying exactly in cell faces: two coordinates multiples of h, along the third axis; and in one face, oblique
        o, d = [], []
        for k in range(3):
            for i in range(0, 5):
                for j in range(0, 4):
                    p = np.array([F(i) * H, F(j) * H, F(i) * H], F)
                    p[k] = F(-0.4)
                    e = np.zeros(3, F)
                    e[k] = 1.0
                    o.append(p), d.append(e)
                    e2 = e.copy()
                    e2[(k + 1) % 3] = 0.25  # stays in the face of axis k + 2
                    o.append(p), d.append(e2)
        return np.array(o, F), np.array(d, F)
    if name == "tie":  # |dx| = |dy| (and |dz|)
        o, d = through(x, rng, 120)
        d[:40, 1] = d[:40, 0]
        d[40:80, 1] = -d[40:80, 0]
        d[80:, 1] = d[80:, 0]
        d[80:, 2] = -d[80:, 0]
        tgt = x[rng.integers(0, len(x), 120)]
        return (tgt - d * F(1.7)).astype(F), d
    if name == "inside_sphere":  # starts inside a sphere: t = ta (0 inside G)
        j = rng.integers(0, len(x), 100)
        o = (x[j].astype(np.float64) + rng.uniform(-0.4, 0.4, (100, 3)) * R0).astype(F)
        return o, rng.normal(size=(100, 3)).astype(F)
    if name == "inside_out":  # starts inside the box, between the particles, and points out
        o = rng.uniform(lo + 0.02, hi - 0.02, (150, 3)).astype(F)
        return o, (o - 0.5 * (lo + hi) + rng.normal(size=(150, 3)) * 0.05).astype(F)
    if name == "away":  # points away from the box: misses
        o, d = through(x, rng, 60)
        return o, (-d).astype(F)
    if name == "far":  # an origin 10^4 h away: the advance
        o, d = through(x, rng, 200)
        n = d / np.linalg.norm(d, axis=1)[:, None]
        return (o - n * F(1.0e4) * H).astype(F), d
    if name == "short_d":
        o, d = through(x, rng, 100)
        return o, (d / np.linalg.norm(d, axis=1)[:, None] * 1.0e-3).astype(F)
    if name == "long_d":
        o, d = through(x, rng, 100)
        return o, (d / np.linalg.norm(d, axis=1)[:, None] * 1.0e3).astype(F)
    if name == "nonfinite":
        o, d = through(x, rng, 70)
        o[3, 1], o[9, 0], d[20, 2], d[31, 0] = np.nan, np.inf, -np.inf, np.nan
        d[40] = 0.0
        d[41] = 1.0e-30  # d.d underflows to 0
        d[42] = 3.0e19   # d.d overflows
        return o, d
    raise KeyError(name)


EDGES = ("axes", "faces", "tie", "inside_sphere", "inside_out", "away", "far", "short_d", "long_d", "nonfinite")


@pytest.mark.parametrize("name", EDGES)
def test_walk_edges(small, name):
    w, _, x, slots = small
    o, d = edge_rays(name, x)
    for R in (R0, float(H) / 2, float(H) / 64):
        ref = rr.cast(o, d, x, slots, R)
        hits = int((ref["row"] >= 0).sum())
        print(name, "R =", R, ":", hits, "hits of", len(o))
        if name == "away":
            assert hits == 0
        elif R >= R0:
            assert hits >= 20
        if name == "inside_sphere" and R >= R0:
            assert (ref["t"] == 0).sum() > 50
        if name == "nonfinite":
            assert (ref["row"][[3, 9, 20, 31, 40, 41, 42]] == -1).all()
        compare(w.cast_rays(o, d, radius=R, normals=True, thickness=True), ref, (name, R))
        compare(w.cast_rays(o, d, radius=R), ref, (name, R, "first hit"))


def test_tmax(small):
    w, _, x, slots = small
    o, d = through(x, np.random.default_rng(23), 200)
    full = rr.cast(o, d, x, slots, R0)
    # per ray a tmax of its own would need a call each: take the rays in three groups with tmax at quantiles of the first hits
    ts = np.sort(full["t"][np.isfinite(full["t"])])
    for tmax in (0.0, float(ts[len(ts) // 4]), float(ts[len(ts) // 2]) * 1.05, float(ts[-1]) * 1.5):
        ref = rr.cast(o, d, x, slots, R0, tmax=tmax)
        compare(w.cast_rays(o, d, tmax=tmax, normals=True, thickness=True), ref, ("tmax", tmax))
    assert (rr.cast(o, d, x, slots, R0, tmax=0.0)["row"] == -1).all()
    # tmax cutting between the first and the second sphere of one ray, and inside the first
    k = int(np.argmax(full["n"] >= 2))
    t0, t1 = rr.cast_f64(o[k:k + 1], d[k:k + 1], x, R0)[2:]
    first = int(np.nanargmin(t0[0]))
    order = np.sort(t0[0][np.isfinite(t0[0])])
    for tmax in (0.5 * (order[0] + order[1]), 0.5 * (t0[0][first] + t1[0][first])):
        ref = rr.cast(o[k:k + 1], d[k:k + 1], x, slots, R0, tmax=tmax)
        assert ref["row"][0] == full["row"][k] and ref["thickness"][0] < full["thickness"][k]
        compare(w.cast_rays(o[k:k + 1], d[k:k + 1], tmax=tmax, normals=True, thickness=True), ref, ("cut", tmax))
    # tmax = 0 from inside a sphere is a hit at t = 0
    inside = x[5:6] + F(0.2 * R0)
    got = w.cast_rays(inside, np.float32([[0.3, 1.0, -0.2]]), tmax=0.0, thickness=True)
    assert got["t"][0] == 0 and got["thickness"][0] == 0
    compare(got, rr.cast(inside, np.float32([[0.3, 1.0, -0.2]]), x, slots, R0, tmax=0.0))


def test_coincident_particles_tie(small):
    """fluid 0's row 7 and fluid 1's rows 4 and 5 sit at the same place: the lower slot wins, and with fluid 0 masked out the lower index"""
    w, (f0, f1), x, slots = small
    o = (x[7] + np.float32([[0.3, 0.01, 0.0], [0.0, -0.3, 0.005], [0.004, 0.002, 0.4]])).astype(F)
    d = (x[7] - o).astype(F)
    got = w.cast_rays(o, d, normals=True, thickness=True)
    ref = rr.cast(o, d, x, slots, R0)
    compare(got, ref)
    hit7 = ref["row"] == 7
    assert hit7.any() and (got["fluid"][hit7] == 0).all() and (got["index"][hit7] == 7).all()
    one = w.cast_rays(o, d, fluids=[f1], normals=True, thickness=True)
    compare(one, rr.cast(o, d, x[slots == 1], slots[slots == 1], R0))
    assert (one["fluid"][hit7] == 1).all() and (one["index"][hit7] == 4).all()


def test_crowded_cell(small):
    w, _, x, slots = small
    crowd = x[-500:]
    o, d = through(crowd, np.random.default_rng(31), 150)
    ref = rr.cast(o, d, x, slots, R0)
    assert ref["n"].max() > 60
    compare(w.cast_rays(o, d, normals=True, thickness=True), ref, "crowd")


def test_clip_box(small):
    """A clip box through the middle of the block: the particles outside it are invisible, those on its faces count."""
    w, _, x, slots = small
    o, d = through(x, np.random.default_rng(37), 300)
    lo, hi = x.min(axis=0), x.max(axis=0)
    clip = (lo.copy(), hi.copy())
    clip[1][0] = x[60, 0]  # a face through a particle: closed
    ref = rr.cast(o, d, x, slots, R0, clip=clip)
    full = rr.cast(o, d, x, slots, R0)
    assert (ref["row"] != full["row"]).sum() > 20 and (ref["row"] >= 0).sum() > 50
    compare(w.cast_rays(o, d, clip=clip, normals=True, thickness=True), ref, "clip")
    # a clip box far larger than the fluid changes nothing but the advance: compared with its own reading
    wide = (lo - F(0.7), hi + F(0.9))
    compare(w.cast_rays(o, d, clip=wide, normals=True, thickness=True), rr.cast(o, d, x, slots, R0, clip=wide), "wide clip")
    # an empty selection box
    empty = (hi + F(1.0), hi + F(2.0))
    got = w.cast_rays(o, d, clip=empty, normals=True, thickness=True)
    assert np.isinf(got["t"]).all() and (got["fluid"] == 0xFFFFFFFF).all() and (got["index"] == 0xFFFFFFFF).all()
    assert (got["normal"] == 0).all() and (got["thickness"] == 0).all()
    # a degenerate clip box: one point, a particle's position
    point = (x[60].copy(), x[60].copy())
    ref = rr.cast(o, d, x, slots, R0, clip=point)
    compare(w.cast_rays(o, d, clip=point, normals=True, thickness=True), ref, "point clip")


@pytest.mark.parametrize("m", [1, 63, 64, 65])
def test_ray_counts(small, m):
    w, _, x, slots = small
    o, d = through(x, np.random.default_rng(41), m)
    compare(w.cast_rays(o, d, normals=True, thickness=True), rr.cast(o, d, x, slots, R0), m)


def test_fluid_mask(world, case):
    w, (f0, f1) = world
    o, d, x, slots, n0 = case["origins"][:1024], case["directions"][:1024], case["x"], case["slots"], case["n0"]
    compare(w.cast_rays(o, d, fluids=[f0], normals=True, thickness=True), rr.cast(o, d, x[:n0], slots[:n0], R0), "fluid 0")
    ref1 = rr.cast(o, d, x[n0:], slots[n0:], R0)
    got1 = w.cast_rays(o, d, fluids=[1], normals=True, thickness=True)
    compare(got1, ref1, "fluid 1")
    assert (got1["fluid"][ref1["row"] >= 0] == 1).all()


def test_empty_world_and_fluid(hip_lib):
    """no particle at all, and a selected fluid whose positions are all non-finite: every ray misses"""
    x = np.full((5, 3), np.nan, F)
    w, _ = rr.make_world(x, np.zeros(5, np.uint32))
    got = w.cast_rays(np.zeros((9, 3), F), np.ones((9, 3), F), normals=True, thickness=True)
    assert np.isinf(got["t"]).all() and (got["index"] == 0xFFFFFFFF).all() and (got["thickness"] == 0).all() and (got["normal"] == 0).all()


# ------------------------------------------------------------------------------------------------ state
def test_state_is_untouched(hip_lib):
    """A world that casts before its first step and between steps, and a twin that never does: the same bits after 20 steps; and the
    casts see the particles as get_fluid returns them."""
    from salva_amd import DFSPHSolver, Fluid, LiquidWorld

    rng = np.random.default_rng(2)
    ix, iy, iz = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    block = (np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1) * (2.0 * R0) + rng.uniform(-0.1, 0.1, (512, 3)) * R0).astype(F)
    worlds = []
    for _ in range(2):
        w = LiquidWorld(DFSPHSolver(), R0, 2.0)
        worlds.append((w, w.add_fluid(Fluid(block.copy(), R0, 1000.0))))
    (w, f), (twin, ft) = worlds
    o, d = through(block, rng, 256)
    slots = np.zeros(512, np.uint32)
    for step in range(20):
        if step in (0, 7, 13):
            x = np.array(f.positions, F)
            compare(w.cast_rays(o, d, normals=True, thickness=True), rr.cast(o, d, x, slots, R0), ("step", step))
        w.step(rc.DT, rc.GRAVITY)
        twin.step(rc.DT, rc.GRAVITY)
    assert np.array_equal(np.array(f.positions, F).view(np.uint32), np.array(ft.positions, F).view(np.uint32))
    assert np.array_equal(np.array(f.velocities, F).view(np.uint32), np.array(ft.velocities, F).view(np.uint32))


# ------------------------------------------------------------------------------------------------ other checks
def test_device_pointers(hip_lib, tmp_path):
    """Rays and outputs in torch tensors on the device (data_ptr()), both flags: the bits are those of the host-pointer call.  In a
    child process, so that torch is loaded before the library (one HIP runtime per process)."""
    out = str(tmp_path / "device.npz")
    r = subprocess.run([sys.executable, os.path.join(TESTS, "fluid_ray_child.py"), "device", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    s = dict(np.load(out))
    for where in ("rays", "camera"):
        for k in rc.OUTPUTS:
            dev, host = s[f"dev_{where}_{k}"], s[f"host_{where}_{k}"]
            assert np.array_equal(dev.view(np.uint32).reshape(-1), host.view(np.uint32).reshape(-1)), (where, k)
        assert np.isfinite(s[f"host_{where}_t"]).sum() > 100


def raw_rays(w, mask, params, o, d, out, flags=0, n=None):
    o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
    fp = C.POINTER(C.c_float)
    return w._L.salva_hip_cast_rays(w._h, mask, C.byref(params) if params is not None else None, len(o) if n is None else n, o.ctypes.data_as(fp),
                                    d.ctypes.data_as(fp), flags, C.byref(out) if out is not None else None)


def raw_camera(w, mask, params, cam, out, flags=0):
    return w._L.salva_hip_cast_rays_camera(w._h, mask, C.byref(params) if params is not None else None, C.byref(cam) if cam is not None else None,
                                           flags, C.byref(out) if out is not None else None)


def raw_count(w, mask, params, cam, o, d, tested, flags=0, walk=0):
    o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
    fp = C.POINTER(C.c_float)
    return w._L.salva_hip_count_ray_candidates(w._h, mask, C.byref(params) if params is not None else None, C.byref(cam) if cam is not None else None,
                                               len(o), o.ctypes.data_as(fp), d.ctypes.data_as(fp), flags, walk,
                                               tested.ctypes.data_as(C.POINTER(C.c_uint32)) if tested is not None else None)


def test_every_refusal_leaves_a_world_that_steps(hip_lib, case):
    """Every refusal on a world of its own, and after each of them a step that completes."""
    from salva_amd import dist

    x, slots = small_scene()
    x, slots = x[:130], slots[:130]  # the block and a few particles of fluid 1
    w, _ = rr.make_world(x, slots)
    w.sync_to_device()  # (the raw calls below do not go through the mirror)
    o, d = through(x, np.random.default_rng(43), 16)
    t = np.zeros(4096, F)
    tested = np.zeros(4096, np.uint32)
    out = _lib.RayOut()
    out.t = t.ctypes.data_as(C.POINTER(C.c_float))
    good = w._ray_params(None, np.inf, None)
    cam = w._ray_camera(case["camera"])
    steps = [0]

    def refused(world, rcode, text, code=_lib.E_INVALID):
        assert rcode == code and text in last_error(), (rcode, text, last_error())
        before = world._nsteps
        assert world.step(rc.DT, (0.0, 0.0, 0.0)) is not None and world._nsteps == before + 1, text
        steps[0] += 1

    assert raw_rays(w, 3, good, o, d, out) == _lib.OK and raw_camera(w, 3, good, cam, out) == _lib.OK
    assert raw_count(w, 3, good, None, o, d, tested) == _lib.OK and raw_count(w, 3, good, cam, o, d, tested, walk=1) == _lib.OK
    refused(w, raw_rays(w, 3, good, o, d, None), "")
    refused(w, raw_rays(w, 3, None, o, d, out), "")
    refused(w, raw_camera(w, 3, good, None, out), "")
    refused(w, raw_count(w, 3, good, None, o, d, None), "")
    refused(w, raw_count(w, 3, good, None, o, d, tested, walk=2), "thickness_walk")
    refused(w, raw_count(w, 3, good, cam, o, d, tested, flags=_lib.RAY_RAYS_ON_DEVICE), "unknown flag")
    refused(w, raw_rays(w, 3, good, o, d, out, flags=4), "unknown flag")
    refused(w, raw_camera(w, 3, good, cam, out, flags=4), "unknown flag")
    refused(w, raw_camera(w, 3, good, cam, out, flags=_lib.RAY_RAYS_ON_DEVICE), "unknown flag")
    refused(w, raw_rays(w, 0b100, good, o, d, out), "selects no existing fluid")
    refused(w, raw_rays(w, 0, good, o, d, out), "selects no existing fluid")
    refused(w, raw_camera(w, 0b100, good, cam, out), "selects no existing fluid")
    fp = C.POINTER(C.c_float)
    refused(w, w._L.salva_hip_cast_rays(w._h, 3, C.byref(good), 4, None, d.ctypes.data_as(fp), 0, C.byref(out)), "null origins or directions")
    refused(w, w._L.salva_hip_cast_rays(w._h, 3, C.byref(good), 4, o.ctypes.data_as(fp), None, 0, C.byref(out)), "null origins or directions")
    assert w._L.salva_hip_cast_rays(w._h, 3, C.byref(good), 0, None, None, 0, C.byref(out)) == _lib.OK  # nrays == 0: nothing to do
    for field, value in (("struct_size", 60), ("version", 2)):
        p = w._ray_params(None, np.inf, None)
        setattr(p, field, value)
        refused(w, raw_rays(w, 3, p, o, d, out), "struct_size / version")
        refused(w, raw_camera(w, 3, p, cam, out), "struct_size / version")
        c = w._ray_camera(case["camera"])
        setattr(c, field, value)
        refused(w, raw_camera(w, 3, good, c, out), "struct_size / version")
    for radius in (0.0, -0.01, float("nan"), float("inf"), float(H) * 0.5001):
        refused(w, raw_rays(w, 3, w._ray_params(radius, np.inf, None), o, d, out), "radius")
    assert raw_rays(w, 3, w._ray_params(float(H) / 2, np.inf, None), o, d, out) == _lib.OK
    for tmax in (-1.0e-9, float("nan"), -float("inf")):
        refused(w, raw_rays(w, 3, w._ray_params(None, tmax, None), o, d, out), "tmax")
    for clip in (([0, 0, 0.2], [1, 1, 0.1]), ([0, np.nan, 0], [1, 1, 1]), ([0, 0, 0], [1, np.inf, 1]), ([-np.inf, 0, 0], [1, 1, 1])):
        refused(w, raw_rays(w, 3, w._ray_params(None, np.inf, clip), o, d, out), "clip box")
    p = w._ray_params(None, np.inf, None)
    p.has_clip = 2
    refused(w, raw_rays(w, 3, p, o, d, out), "has_clip")
    for dims in ((0, 4), (4, 0)):
        c = w._ray_camera(dict(case["camera"], width=dims[0], height=dims[1]))
        refused(w, raw_camera(w, 3, good, c, out), "width and height")
    # more than 2^32 rays: refused before anything is read or written, from a list and from a camera
    refused(w, raw_rays(w, 3, good, o, d, out, n=(1 << 32) + 1), "2^32 rays", _lib.E_CAPACITY)
    huge = w._ray_camera(dict(case["camera"], width=1 << 17, height=(1 << 15) + 1))
    refused(w, raw_camera(w, 3, good, huge, out), "2^32 rays", _lib.E_CAPACITY)
    with pytest.raises(_lib.SalvaHipError) as e:  # (the mirror hands the library's refusal on)
        w.cast_camera(dict(case["camera"], width=1 << 17, height=(1 << 15) + 1))
    assert e.value.code == _lib.E_CAPACITY and "2^32 rays" in str(e.value)
    assert steps[0] == w._nsteps and raw_rays(w, 3, good, o, d, out) == _lib.OK
    # a loopback-decomposed world
    wd, _ = rr.make_world(x, slots)
    cx = dist.cell_x(x, wd.h())
    wd.set_domain(dist.Comm.loopback(1)[0], int(cx.min()), int(cx.max()), 0)
    wd.step(rc.DT, (0.0, 0.0, 0.0))
    refused(wd, raw_rays(wd, 3, good, o, d, out), "host-order arrays are not maintained")
    refused(wd, raw_camera(wd, 3, good, cam, out), "host-order arrays are not maintained")
    refused(wd, raw_count(wd, 3, good, None, o, d, tested), "host-order arrays are not maintained")


def test_candidate_counts(small):
    """salva_hip_count_ray_candidates: the thickness walk tests at least every particle the reading's ray meets at t1 >= 0, the
    first-hit walk at least one where there is a hit and never more than the thickness walk, a ray that misses the box none; the
    camera's counts are those of the same rays from a list."""
    w, _, x, slots = small
    o, d = through(x, np.random.default_rng(53), 300)
    d[20:30] = -d[20:30]  # (these point away from the box)
    ref = rr.cast(o, d, x, slots, R0)
    first, thick = w.count_ray_candidates(o, d), w.count_ray_candidates(o, d, thickness_walk=True)
    assert first.dtype == np.uint32 and first.shape == (300,)
    live = rr.advance(o, d, rr.grown(rr.bounds(x), R0), np.inf)[0]
    assert (first[~live] == 0).all() and (thick[~live] == 0).all() and (~live).sum() >= 10
    assert (first <= thick).all() and (first[ref["row"] >= 0] >= 1).all() and (first < thick).any()
    tm, p, t0, t1 = rr.cast_f64(o, d, x, R0)
    sure = ((p < R0 * (1 - 1e-3)) & (t1 > 1e-3)).sum(axis=1)  # clearly met, clearly in front
    assert (thick >= sure).all() and thick.max() < len(x)
    cam = {"origin": x.mean(axis=0) + F([0.02, 0.9, -0.01]), "forward": [0.0, -1.0, 0.0], "right": [0.3, 0.0, 0.0], "up": [0.0, 0.0, 0.25],
           "width": 13, "height": 9}
    co, cd = rr.camera_rays(cam)
    for walk in (False, True):
        assert np.array_equal(w.count_ray_candidates(camera=cam, thickness_walk=walk).reshape(-1), w.count_ray_candidates(co, cd, thickness_walk=walk))


def test_refused_inside_a_force_callback(hip_lib):
    from salva_amd import NonPressureForce

    x, slots = small_scene()
    w, (f0, _) = rr.make_world(x, slots)

    class Calls(NonPressureForce):
        def solve(self, timestep, kernel_radius, ff, fb, fluid, boundaries, densities):
            t = np.zeros(8, F)
            out = _lib.RayOut()
            out.t = t.ctypes.data_as(C.POINTER(C.c_float))
            p = self.world._ray_params(None, np.inf, None)
            cam = self.world._ray_camera({"origin": [0, 0, 1], "forward": [0, 0, -1], "right": [1, 0, 0], "up": [0, 1, 0], "width": 2, "height": 2})
            self.seen = (raw_rays(self.world, 3, p, np.zeros((8, 3), F), np.ones((8, 3), F), out), last_error(),
                         raw_camera(self.world, 3, p, cam, out), last_error())

    force = Calls()
    force.world = w
    f0.nonpressure_forces.append(force)
    st = w.step(rc.DT, (0.0, 0.0, 0.0))
    assert force.seen[0] == _lib.E_INVALID and force.seen[2] == _lib.E_INVALID and "callback" in force.seen[1] and "callback" in force.seen[3]
    assert st is not None and w._nsteps == 1  # the step completed


def test_capacity_names_the_clip_box(small):
    """One stray particle a million cells away: without a clip box the table would not fit, and the message says what to do; with one
    the call succeeds and sees what the reading sees."""
    _, _, x, slots = small
    stray = np.float32([[1.0e6 * float(H), 0.05, 0.05]])
    xs, ss = np.concatenate([x, stray]), np.concatenate([slots, np.ones(1, np.uint32)])
    w, _ = rr.make_world(xs, ss)
    o, d = through(x, np.random.default_rng(47), 64)
    with pytest.raises(_lib.SalvaHipError) as e:
        w.cast_rays(o, d)
    assert e.value.code == _lib.E_CAPACITY and "give a clip box" in str(e.value)
    clip = (x.min(axis=0), x.max(axis=0))
    ref = rr.cast(o, d, xs, ss, R0, clip=clip)
    compare(w.cast_rays(o, d, clip=clip, normals=True, thickness=True), ref, "stray")
    compare({k: v for k, v in ref.items() if k in rc.OUTPUTS}, rr.cast(o, d, x, slots, R0, clip=clip))
    assert w.step(rc.DT, (0.0, 0.0, 0.0)) is not None


def test_depth_image3_example_agrees_with_the_python_mirror(hip_lib):
    """examples/depth_image3.cpp prints the hit count, the sums and minima of its depth and thickness images; the Python mirror on the
    same scene gives the same numbers (the sums are taken in f64 over the same f32 images)."""
    import re

    root = os.path.dirname(TESTS)
    exe = os.path.join(root, "examples", "depth_image3")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "examples"), "depth_image3"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"hits (\d+) of (\d+); depth sum ([-0-9.eE+]+) min ([-0-9.eE+]+); thickness sum ([-0-9.eE+]+) min ([-0-9.eE+]+)", r.stdout)
    assert m, r.stdout
    hits, dsum, dmin, tsum, tmin = rc.depth_image3()
    assert (int(m.group(1)), int(m.group(2))) == (hits, 64 * 48) and hits > 200
    assert float(m.group(3)) == pytest.approx(dsum, rel=1e-12) and float(m.group(4)) == pytest.approx(dmin, rel=1e-7)
    assert float(m.group(5)) == pytest.approx(tsum, rel=1e-12) and float(m.group(6)) == pytest.approx(tmin, rel=1e-7)
