"""The surface extractor (salva_hip_extract_surface / _from_values, salva_hip_get_fluid_bounds) on the device against
the numpy reading tests/surface_reading.py: counts and triangle indices exactly, vertex positions bit for bit.  Jobs that need a
process of their own (an environment switch, torch before the library, twin worlds) run in fresh children (tests/surface_child.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import field_child as fc
import field_reading as fr
import surface_child as sc
import surface_reading as sr
from salva_amd import _lib

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24
CANARY = 0x7FC0BEEF
LATTICES = {"random": (sr.random_lattice, 0.5), "linear": (sr.linear_lattice, sr.LINEAR_ISO)}


@pytest.fixture(scope="module")
def case():
    return fr.standard_case()


@pytest.fixture(scope="module")
def small_world(hip_lib):
    """a world without particles: enough for a caller's lattice"""
    from salva_amd import DFSPHSolver, LiquidWorld

    return LiquidWorld(DFSPHSolver(), 0.025, 2.0)


@pytest.fixture(scope="module")
def readings():
    """the reading of the two small lattices, shared and left unchanged"""
    return {name: sr.extract(make(), iso, sr.LATTICE_ORIGIN, sr.LATTICE_SPACING) for name, (make, iso) in LATTICES.items()}


def child(job, tmp_path, **env):
    out = str(tmp_path / (job + ".npz"))
    e = dict(os.environ)
    for k in ("SALVA_HIP_FIELD_ARM", "SALVA_HIP_FOLD_CELLS", "SALVA_HIP_NO_FOLD"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(TESTS, "surface_child.py"), job, out], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def device_meshes(tmp_path_factory):
    return child("device", tmp_path_factory.mktemp("device"))


@pytest.fixture(scope="module")
def arms(tmp_path_factory):
    d = tmp_path_factory.mktemp("arms")
    out = {}
    for arm in ("points", "lattice"):
        (d / arm).mkdir()
        out[arm] = child("arms", d / arm, SALVA_HIP_FIELD_ARM=arm)
    return out


def same_mesh(got_v, got_t, ref_v, ref_t):
    assert got_t.shape == ref_t.shape and got_v.shape == ref_v.shape, (got_v.shape, got_t.shape, ref_v.shape, ref_t.shape)
    assert np.array_equal(got_t, ref_t)
    assert np.array_equal(np.ascontiguousarray(got_v).view(np.uint32), np.ascontiguousarray(ref_v).view(np.uint32))  # bit for bit


def last_error():
    return _lib.lib().salva_hip_last_error().decode()


def u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def raw_values(w, values, iso, out, counts, origin=sr.LATTICE_ORIGIN, spacing=sr.LATTICE_SPACING, dims=None, flags=0):
    v = np.ascontiguousarray(values, np.float32)
    o = np.ascontiguousarray(origin, np.float32)
    d = np.ascontiguousarray(v.shape if dims is None else dims, np.uint32)
    return w._L.salva_hip_extract_surface_from_values(w._h, f32p(v), float(iso), f32p(o), float(spacing), u32p(d), flags,
                                                      C.byref(out) if out is not None else None, counts)


def raw_field(w, mask, field, iso, origin, spacing, dims, out, counts, flags=0):
    o, d = np.ascontiguousarray(origin, np.float32), np.ascontiguousarray(dims, np.uint32)
    return w._L.salva_hip_extract_surface(w._h, mask, field, float(iso), f32p(o), float(spacing), u32p(d), flags,
                                          C.byref(out) if out is not None else None, counts)


def canary_out(nv, nt, vcap=None, tcap=None):
    bufs = {"vertices": np.full(3 * nv + 3, CANARY, np.uint32), "triangles": np.full(3 * nt + 3, CANARY, np.uint32)}
    out = _lib.SurfaceOut()
    out.vertices, out.triangles = f32p(bufs["vertices"]), u32p(bufs["triangles"])
    out.vertex_capacity, out.triangle_capacity = nv if vcap is None else vcap, nt if tcap is None else tcap
    return bufs, out


# 1, 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LATTICES))
def test_supplied_lattice_from_host_and_device_memory(small_world, readings, device_meshes, name):
    make, iso = LATTICES[name]
    ref_v, ref_t, seen = readings[name]
    if name == "random":
        assert len(seen) == 84  # every case of the table runs
    got = small_world.extract_surface_from_values(make(), sr.LATTICE_ORIGIN, sr.LATTICE_SPACING, iso)
    same_mesh(got["vertices"], got["triangles"], ref_v, ref_t)
    again = small_world.extract_surface_from_values(make(), sr.LATTICE_ORIGIN, sr.LATTICE_SPACING, iso)
    same_mesh(again["vertices"], again["triangles"], got["vertices"], got["triangles"])
    same_mesh(device_meshes[name + "_vertices"], device_meshes[name + "_triangles"], ref_v, ref_t)


# 3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["points", "lattice"])
@pytest.mark.parametrize("field,iso", sc.SURFACES)
def test_surface_of_the_standard_world(case, arms, field, iso, arm):
    s = arms[arm]
    lattice = s[field + "_lattice"]
    assert lattice.shape == case["dims"]
    ref_v, ref_t, _ = sr.extract(lattice, iso, case["origin"], case["spacing"])
    v, t = s[field + "_vertices"], s[field + "_triangles"]
    same_mesh(v, t, ref_v, ref_t)
    unique, open_edges = sr.edge_report(t)
    assert unique and len(open_edges) == 0
    assert sr.euler_characteristic(len(v), t) == 2
    volume = sr.signed_volume(v, t)
    print(f"{field} / {arm}: {len(v)} vertices, {len(t)} triangles, volume {volume:.4f}")
    assert volume > 0.0


# 4 ------------------------------------------------------------------------------------------------
def test_fluid_mask(hip_lib, case):
    w, (f0, _) = fc.standard_world(case)
    lattice = w.evaluate_lattice(case["origin"], case["spacing"], case["dims"], fluids=[f0], density=False, fraction=True)["fraction"]
    ref_v, ref_t, _ = sr.extract(lattice, 0.5, case["origin"], case["spacing"])
    one = w.extract_surface(case["origin"], case["spacing"], case["dims"], fluids=[f0])
    same_mesh(one["vertices"], one["triangles"], ref_v, ref_t)
    both = w.extract_surface(case["origin"], case["spacing"], case["dims"])
    assert len(both["vertices"]) != len(one["vertices"]) and len(one["vertices"]) > 1000


# 5 ------------------------------------------------------------------------------------------------
def test_normals_and_velocities(hip_lib, case):
    """The velocities are the evaluator's own kernel on the same points: the same bits.  The normal is -g / |g| in f32 with g scaled by
    its largest component first: a rounding in each of the scaling, the three squares (relative to the sum: one), the two sums, the
    root (halved with what is under it) and the final quotient - (1 + (2 + 1 + 2) / 2 + 1 + 1) u = 5.5 u relative to the component,
    asserted as 6 u absolute; the same for the length."""
    w, _ = fc.standard_world(case)
    mesh = w.extract_surface(case["origin"], case["spacing"], case["dims"], normals=True, velocities=True)
    v, t, n = mesh["vertices"], mesh["triangles"].astype(np.int64), mesh["normals"]
    ref = w.evaluate_fields(v, density=False, velocity=True, gradient=True)
    assert np.array_equal(mesh["velocities"].view(np.uint32), ref["velocity"].view(np.uint32))
    assert np.abs(mesh["velocities"]).max() > 0.1
    g = ref["gradient"].astype(np.float64)
    length = np.linalg.norm(g, axis=1)
    zero = length == 0.0
    assert (n[zero] == 0.0).all() and (~zero).mean() > 0.99
    want = -g[~zero] / length[~zero, None]
    err = np.abs(n[~zero].astype(np.float64) - want).max()
    print(f"worst normal component error: {err / U:.2f} u")
    assert err <= 6.0 * U
    assert np.abs(np.linalg.norm(n[~zero].astype(np.float64), axis=1) - 1.0).max() <= 6.0 * U
    p = v.astype(np.float64)[t]
    geometric = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    mean = n.astype(np.float64)[t].mean(axis=1)
    assert (np.einsum("ij,ij->i", geometric, mean) > 0.0).all()


# 6 ------------------------------------------------------------------------------------------------
def test_counts_and_capacity(small_world, readings):
    w = small_world
    values = sr.random_lattice()
    ref_v, ref_t, _ = readings["random"]
    nv, nt = len(ref_v), len(ref_t)
    counts = (C.c_uint64 * 2)()
    assert raw_values(w, values, 0.5, None, counts) == _lib.OK and (counts[0], counts[1]) == (nv, nt)  # count only
    for vcap, tcap in ((nv - 1, nt), (nv, nt - 1)):
        bufs, out = canary_out(nv, nt, vcap, tcap)
        counts = (C.c_uint64 * 2)()
        assert raw_values(w, values, 0.5, out, counts) == _lib.E_CAPACITY, last_error()
        assert (counts[0], counts[1]) == (nv, nt)
        assert all((b == CANARY).all() for b in bufs.values())
    bufs, out = canary_out(nv, nt)
    assert raw_values(w, values, 0.5, out, counts) == _lib.OK, last_error()
    same_mesh(bufs["vertices"][:3 * nv].view(np.float32).reshape(nv, 3), bufs["triangles"][:3 * nt].reshape(nt, 3), ref_v, ref_t)
    assert (bufs["vertices"][3 * nv:] == CANARY).all() and (bufs["triangles"][3 * nt:] == CANARY).all()


# 7 ------------------------------------------------------------------------------------------------
def test_refusals(hip_lib, small_world, case):
    from salva_amd import dist

    w = small_world
    values = sr.random_lattice()
    counts = (C.c_uint64 * 2)()
    bufs, out = canary_out(400, 800)

    def untouched():
        return all((b == CANARY).all() for b in bufs.values())

    for iso in (float("nan"), float("inf"), float("-inf")):
        assert raw_values(w, values, iso, out, counts) == _lib.E_INVALID and "iso" in last_error()
    for dims in ((1, 6, 5), (7, 1, 5), (7, 6, 1), (0, 6, 5)):
        assert raw_values(w, values, 0.5, out, counts, dims=dims) == _lib.E_INVALID and "at least 2" in last_error()
    for spacing in (0.0, -1.0, float("nan"), float("inf")):
        assert raw_values(w, values, 0.5, out, counts, spacing=spacing) == _lib.E_INVALID and "spacing" in last_error()
    assert raw_values(w, values, 0.5, out, counts, flags=4) == _lib.E_INVALID and "unknown flag" in last_error()
    assert raw_values(w, values, 0.5, out, None) == _lib.E_INVALID  # null counts
    # normals and velocities of a supplied lattice
    spare = np.zeros(3 * 400, np.float32)
    for name in ("normals", "velocities"):
        _, o2 = canary_out(400, 800)
        setattr(o2, name, f32p(spare))
        assert raw_values(w, values, 0.5, o2, counts) == _lib.E_INVALID and "must be NULL" in last_error()
    # a node value that is not finite
    for bad in (np.nan, np.inf, -np.inf):
        v = values.copy()
        v[3, 2, 4] = bad
        assert raw_values(w, v, 0.5, out, counts) == _lib.E_INVALID and "not finite" in last_error()
        assert raw_values(w, v, 0.5, None, counts) == _lib.E_INVALID
    # too many nodes (refused before `values` is read)
    assert raw_values(w, values, 0.5, out, counts, dims=(1 << 11, 1 << 10, 1 << 10)) == _lib.E_CAPACITY and "nodes" in last_error()
    assert raw_values(w, values, 0.5, out, counts, dims=(1 << 16, 1 << 16, 2)) == _lib.E_CAPACITY
    assert untouched()
    # the field entry: its own arguments, and the evaluator's refusals
    ws, _ = fc.standard_world(case)
    assert ws.fluid_bounds()[2] == len(case["x"])  # (through the mirror: the fluids are on the device from here on)
    o, s, d = case["origin"], case["spacing"], case["dims"]
    assert raw_field(ws, 3, _lib.SURFACE_FRACTION, 0.5, o, s, d, None, counts) == _lib.OK and counts[0] > 1000
    assert raw_field(ws, 3, 2, 0.5, o, s, d, out, counts) == _lib.E_INVALID and "unknown field" in last_error()
    assert raw_field(ws, 3, _lib.SURFACE_FRACTION, 0.5, o, s, d, out, counts, flags=_lib.SURFACE_VALUES_ON_DEVICE) == _lib.E_INVALID
    assert "unknown flag" in last_error()
    assert raw_field(ws, 3, _lib.SURFACE_FRACTION, float("nan"), o, s, d, out, counts) == _lib.E_INVALID
    assert raw_field(ws, 3, _lib.SURFACE_FRACTION, 0.5, o, s, (39, 1, 29), out, counts) == _lib.E_INVALID
    assert raw_field(ws, 3, _lib.SURFACE_FRACTION, 0.5, o, -1.0, d, out, counts) == _lib.E_INVALID
    assert raw_field(ws, 0b100, _lib.SURFACE_FRACTION, 0.5, o, s, d, out, counts) == _lib.E_INVALID and "selects no existing fluid" in last_error()
    lo, hi, n = np.zeros(3, np.float32), np.zeros(3, np.float32), C.c_uint64(0)
    assert ws._L.salva_hip_get_fluid_bounds(ws._h, 0, f32p(lo), f32p(hi), C.byref(n)) == _lib.E_INVALID
    assert raw_field(ws, 3, _lib.SURFACE_FRACTION, 0.5, o, s, d, out, counts) == _lib.E_CAPACITY and counts[0] > 400  # (room for 400)
    assert untouched()
    # a loopback-decomposed world
    wd, _ = fc.standard_world(case)
    wd.set_domain(dist.Comm.loopback(1)[0], -1000, 1000)
    assert raw_field(wd, 3, _lib.SURFACE_FRACTION, 0.5, o, s, d, out, counts) == _lib.E_INVALID and "host-order arrays are not maintained" in last_error()
    assert wd._L.salva_hip_get_fluid_bounds(wd._h, 3, f32p(lo), f32p(hi), C.byref(n)) == _lib.E_INVALID
    assert untouched()


def test_refused_inside_a_force_callback(hip_lib, case):
    from salva_amd import NonPressureForce

    class Calls(NonPressureForce):
        def solve(self, timestep, kernel_radius, ff, fb, fluid, boundaries, densities):
            counts = (C.c_uint64 * 2)()
            lo, hi, n = np.zeros(3, np.float32), np.zeros(3, np.float32), C.c_uint64(0)
            w = self.world
            self.seen = [(raw_field(w, 3, _lib.SURFACE_FRACTION, 0.5, (0, 0, 0), 0.1, (2, 2, 2), None, counts), last_error()),
                         (raw_values(w, np.zeros((2, 2, 2), np.float32), 0.5, None, counts), last_error()),
                         (w._L.salva_hip_get_fluid_bounds(w._h, 3, f32p(lo), f32p(hi), C.byref(n)), last_error())]

    w, (f0, _) = fc.standard_world(case)
    force = Calls()
    force.world = w
    f0.nonpressure_forces.append(force)
    st = w.step(fc.DT, (0.0, 0.0, 0.0))
    for rc, message in force.seen:
        assert rc == _lib.E_INVALID and "callback" in message
    assert st is not None and w._nsteps == 1  # the step completed


# 8 ------------------------------------------------------------------------------------------------
def test_state(hip_lib, tmp_path):
    """A twin world that never extracts has the same bits after 20 steps."""
    s = child("state", tmp_path)
    assert s["nv"] > 100 and s["nt"] > 100
    assert np.array_equal(s["end_x"], s["twin_x"]) and np.array_equal(s["end_v"], s["twin_v"])


# 9 ------------------------------------------------------------------------------------------------
def test_fluid_bounds_and_surface_lattice(hip_lib, case):
    x1 = case["x"][case["n0"]:].copy()
    x1[7] = (np.nan, 0.1, 0.1)
    x1[11, 2] = np.inf
    extra = np.float32([[5.0, -3.0, 0.25]])
    w, (f0, f1) = fc.standard_world(case, extra=extra)
    f1.positions = np.concatenate([x1, extra])
    x0 = case["x"][:case["n0"]]
    everything = np.concatenate([x0, x1, extra])
    finite = np.isfinite(everything).all(axis=1)
    lo, hi, n = w.fluid_bounds()
    assert n == int(finite.sum()) == len(everything) - 2
    assert np.array_equal(lo, everything[finite].min(axis=0)) and np.array_equal(hi, everything[finite].max(axis=0))
    lo, hi, n = w.fluid_bounds(fluids=[f0])  # the fluid with the stray and the NaN is excluded by the mask
    assert n == len(x0) and np.array_equal(lo, x0.min(axis=0)) and np.array_equal(hi, x0.max(axis=0))
    spacing, margin = np.float32(0.03), 0.07
    origin, dims = w.surface_lattice(spacing, margin=margin, fluids=[f0])
    last = np.array([sr.axis_nodes(origin[a], spacing, dims[a])[-1] for a in range(3)])
    assert (origin.astype(np.float64) <= lo.astype(np.float64) - margin).all() and (last.astype(np.float64) >= hi.astype(np.float64) + margin).all()
    assert (origin.astype(np.float64) > lo.astype(np.float64) - margin - 2.0 * spacing).all()
    k = np.round(origin.astype(np.float64) / float(spacing))
    assert np.array_equal(k.astype(np.float32) * spacing, origin)  # a multiple of the spacing
    assert w.surface_lattice(spacing, fluids=[f0])[0][0] <= float(lo[0]) - w.h()  # the default margin is h


# 10 -----------------------------------------------------------------------------------------------
def test_surface3_example_agrees_with_the_python_mirror(hip_lib, tmp_path):
    """examples/surface3.cpp: the basic3 block after 50 steps, the lattice from fluid_bounds, the surface fraction = 0.5 with normals:
    its counts and its OBJ are the Python mirror's mesh of the same scene."""
    root = os.path.dirname(TESTS)
    exe = os.path.join(root, "examples", "surface3")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "examples"), "surface3"], stdout=subprocess.DEVNULL)
    obj = str(tmp_path / "surface3.obj")
    r = subprocess.run([exe, obj], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"vertices: (\d+); triangles: (\d+); volume ([-0-9.eE+]+); area ([-0-9.eE+]+)", r.stdout)
    assert m, r.stdout
    mesh = sc.surface3()
    v, t, n = mesh["vertices"], mesh["triangles"], mesh["normals"]
    assert (int(m.group(1)), int(m.group(2))) == (len(v), len(t))
    assert abs(float(m.group(3)) - sr.signed_volume(v, t)) <= 1e-5 and abs(float(m.group(4)) - sr.area(v, t)) <= 1e-4
    lines = open(obj).read().split("\n")
    got_v = np.array([l.split()[1:] for l in lines if l.startswith("v ")], np.float32)
    got_n = np.array([l.split()[1:] for l in lines if l.startswith("vn ")], np.float32)
    got_f = np.array([[int(c.split("//")[0]) for c in l.split()[1:]] for l in lines if l.startswith("f ")], np.int64)
    assert np.array_equal(got_v, v) and np.array_equal(got_n, n)  # (printed with nine significant digits: f32 round trip)
    assert np.array_equal(got_f - 1, t.astype(np.int64))
