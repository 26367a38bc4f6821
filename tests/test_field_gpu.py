"""The field evaluator (salva_hip_evaluate_fields / _lattice) on the device against the brute-force reading
tests/field_reading.py at its derived tolerance (n + 16) 2^-24 A — see the reading's docstring; counts and exact zeros are compared
exactly.  Jobs that need an environment switch of their own run in fresh child processes (tests/field_child.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import field_child as fc
import field_reading as fr
from salva_amd import _lib

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
BORDER = 1.0e-4 * fr.R


@pytest.fixture(scope="module")
def case():
    return fr.standard_case()


@pytest.fixture(scope="module")
def pairs(case):
    """the pair lists of the standard case, shared and left unchanged"""
    return {"points": fr.find_pairs(case["points"], case["x"], case["h"], BORDER), "nodes": fr.find_pairs(case["nodes"], case["x"], case["h"], BORDER)}


def reading(case, pairs, where, kd="cubic", kg="cubic", rows=slice(None)):
    p = pairs[where]
    if rows != slice(None):  # a subset of the particles: its own pairs
        return fr.evaluate(case[where], case["x"][rows], case["v"][rows], case["vol"][rows], case["rho0"][rows], case["h"], fc.KINDS[kd],
                           fc.KINDS[kg], border=BORDER)
    return fr.evaluate(case[where], case["x"], case["v"], case["vol"], case["rho0"], case["h"], fc.KINDS[kd], fc.KINDS[kg], pairs=p)


def child(job, tmp_path, **env):
    out = str(tmp_path / (job + ".npz"))
    e = dict(os.environ)
    for k in ("SALVA_HIP_FIELD_ARM", "SALVA_HIP_FOLD_CELLS", "SALVA_HIP_NO_FOLD"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(TESTS, "field_child.py"), job, out], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def arms(tmp_path_factory):
    """the lattice jobs, one fresh process per forced arm"""
    d = tmp_path_factory.mktemp("arms")
    out = {}
    for arm in ("points", "lattice"):
        (d / arm).mkdir()
        out[arm] = child("arms", d / arm, SALVA_HIP_FIELD_ARM=arm)
    return out


def raw_call(w, mask, pts, out, flags=0):
    p = np.ascontiguousarray(pts, np.float32)
    return w._L.salva_hip_evaluate_fields(w._h, mask, len(p), p.ctypes.data_as(C.POINTER(C.c_float)), flags, C.byref(out) if out is not None else None)


def raw_lattice(w, mask, origin, spacing, dims, out):
    o, d = np.ascontiguousarray(origin, np.float32), np.ascontiguousarray(dims, np.uint32)
    return w._L.salva_hip_evaluate_fields_lattice(w._h, mask, o.ctypes.data_as(C.POINTER(C.c_float)), float(spacing),
                                                  d.ctypes.data_as(C.POINTER(C.c_uint32)), 0, C.byref(out) if out is not None else None)


def last_error():
    return _lib.lib().salva_hip_last_error().decode()


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kd,kg", fc.COMBOS)
def test_every_field_on_the_points(hip_lib, case, pairs, kd, kg):
    w, _ = fc.standard_world(case, kd, kg)
    got = fc.flat(w.evaluate_fields(case["points"], **fc.ALL))
    fr.compare(got, reading(case, pairs, "points", kd, kg))
    again = fc.flat(w.evaluate_fields(case["points"], **fc.ALL))
    for k in got:
        assert np.array_equal(got[k], again[k]), k  # the order of every sum is fixed: the same bits


@pytest.mark.parametrize("arm", ["points", "lattice"])
@pytest.mark.parametrize("kd,kg", fc.COMBOS)
def test_every_field_on_the_lattice(hip_lib, case, pairs, arms, kd, kg, arm):
    got = {k: arms[arm][f"{kd}_{kg}_{k}"] for k in fc.ALL}
    fr.compare(got, reading(case, pairs, "nodes", kd, kg))


# 2 ------------------------------------------------------------------------------------------------
def test_the_two_arms_against_each_other(hip_lib, case, pairs, arms):
    """The lattice's nodes, computed in numpy with the same f32 product and sum, through salva_hip_evaluate_fields."""
    w, _ = fc.standard_world(case)
    pts = fc.flat(w.evaluate_fields(case["nodes"], **fc.ALL))
    ref = reading(case, pairs, "nodes")
    for arm in ("points", "lattice"):
        got = {k: arms[arm][f"cubic_cubic_{k}"] for k in fc.ALL}
        assert np.array_equal(got["count"], pts["count"]), arm
        same = {k: bool(np.array_equal(got[k], pts[k])) for k in fc.ALL}
        print(arm, "arm against the points entry, bit for bit:", same)
        for name, A in (("density", ref["A_density"]), ("fraction", ref["A_fraction"])):
            assert (np.abs(got[name].astype(np.float64) - pts[name]) <= fr.tol_sum(ref["n"], A)).all(), (arm, name)
        assert (np.abs(got["gradient"].astype(np.float64) - pts["gradient"]) <= fr.tol_sum(ref["n"], ref["A_gradient"])[:, None]).all(), arm
        assert (np.abs(got["velocity"].astype(np.float64) - pts["velocity"]) <= fr.tol_velocity(ref)).all(), arm


# 3 ------------------------------------------------------------------------------------------------
def test_fluid_mask(hip_lib, case, pairs):
    w, (f0, f1) = fc.standard_world(case)
    n0 = case["n0"]
    both = fc.flat(w.evaluate_fields(case["points"], **fc.ALL))
    one = fc.flat(w.evaluate_fields(case["points"], fluids=[f0], **fc.ALL))
    two = fc.flat(w.evaluate_fields(case["points"], fluids=[1], **fc.ALL))
    fr.compare(one, reading(case, pairs, "points", rows=slice(0, n0)))
    fr.compare(two, reading(case, pairs, "points", rows=slice(n0, None)))
    ref = reading(case, pairs, "points")
    assert (np.abs(both["density"].astype(np.float64) - (one["density"].astype(np.float64) + two["density"])) <= fr.tol_sum(ref["n"], ref["A_density"])).all()
    assert np.array_equal(both["count"], one["count"] + two["count"])
    out = _lib.FieldOut()
    d = np.zeros(len(case["points"]), np.float32)
    out.density = d.ctypes.data_as(C.POINTER(C.c_float))
    assert raw_call(w, 0b100, case["points"], out) == _lib.E_INVALID and "selects no existing fluid" in last_error()
    assert raw_call(w, 0, case["points"], out) == _lib.E_INVALID
    assert raw_call(w, 0b110, case["points"], out) == _lib.OK  # (an absent fluid beside an existing one is ignored)
    assert np.array_equal(d, two["density"])


# 4 ------------------------------------------------------------------------------------------------
def test_output_subsets(hip_lib, case):
    w, _ = fc.standard_world(case)
    pts, m = case["points"], len(case["points"])
    full = fc.flat(w.evaluate_fields(pts, **fc.ALL))
    widths = dict(density=1, fraction=1, velocity=3, gradient=3, count=1)
    for name in fc.ALL:
        bufs = {k: np.full(m * widths[k], 0x7FC0BEEF, np.uint32) for k in fc.ALL}  # the canary
        out = _lib.FieldOut()
        setattr(out, name, bufs[name].ctypes.data_as(C.POINTER(C.c_uint32 if name == "count" else C.c_float)))
        assert raw_call(w, 3, pts, out) == _lib.OK, last_error()
        assert np.array_equal(bufs[name], full[name].reshape(-1).view(np.uint32)), name
        for k in fc.ALL:
            if k != name:
                assert (bufs[k] == 0x7FC0BEEF).all(), (name, k)


# 5 ------------------------------------------------------------------------------------------------
def test_the_solvers_own_numbers(hip_lib, case):
    """count and density at the particles' own positions before the first step against what the step then computes from the same
    positions (one fluid, no boundary)."""
    from salva_amd import DFSPHSolver, Fluid, LiquidWorld

    x = case["x"][:case["n0"]]
    w = LiquidWorld(DFSPHSolver(), case["r"], fr.SMOOTHING)
    f = w.add_fluid(Fluid(x, case["r"], 1000.0))
    got = fc.flat(w.evaluate_fields(x, density=True, count=True))
    w.step(fc.DT, (0.0, 0.0, 0.0))
    assert np.array_equal(got["count"], w.contact_counts(f))  # self included
    vol = np.full(len(x), f.default_particle_volume(), np.float32)
    ref = fr.evaluate(x, x, np.zeros_like(x), vol, np.full(len(x), 1000.0), case["h"])
    err = np.abs(got["density"].astype(np.float64) - w.densities(f))
    print("worst error / tolerance:", float((err / fr.tol_sum(ref["n"], ref["A_density"])).max()))
    assert (err <= fr.tol_sum(ref["n"], ref["A_density"])).all()
    fr.compare(got, ref, fields=("density",))


# 6 ------------------------------------------------------------------------------------------------
def test_crowding_and_coarseness(hip_lib, case, arms):
    """600 particles in one cell beside the standard cloud (several chunks per brick), lattices at spacing h and 3 h on the brick arm."""
    extra = fc.crowd(case)
    x = np.concatenate([case["x"], extra])
    v = np.concatenate([case["v"], np.zeros((len(extra), 3), np.float32)])
    vol = np.concatenate([case["vol"], np.full(len(extra), np.float32(case["r"]) ** 3 * np.float32(6.4), np.float32)])
    rho0 = np.concatenate([case["rho0"], np.full(len(extra), fr.DENSITY0[1])])
    cells = np.floor(extra.astype(np.float64) / case["h"])
    assert (cells == cells[0]).all()
    lattices = fc.coarse_lattices(case) + [(case["origin"], case["spacing"], case["dims"])]
    for n, (origin, spacing, dims) in enumerate(lattices):
        key = f"coarse{n}" if n < 2 else "crowd"
        ref = fr.evaluate(fr.lattice_nodes(origin, spacing, dims), x, v, vol, rho0, case["h"], border=BORDER)
        assert ref["n"].max() >= (600 if n == 2 else 1)
        for arm in ("lattice", "points"):
            fr.compare({k: arms[arm][f"{key}_{k}"] for k in fc.ALL}, ref)


# 7 ------------------------------------------------------------------------------------------------
def test_strays(hip_lib, case):
    w, _ = fc.standard_world(case)
    far = np.float32([[1.0e6 * case["h"], 0.0, 0.0], [0.1, -1.0e6 * case["h"], 0.2], [0.0, 0.0, 3.0e6 * case["h"]]])
    ws, _ = fc.standard_world(case, extra=far)
    for a, b in ((w.evaluate_fields(case["points"], **fc.ALL), ws.evaluate_fields(case["points"], **fc.ALL)),
                 (w.evaluate_lattice(case["origin"], case["spacing"], case["dims"], **fc.ALL),
                  ws.evaluate_lattice(case["origin"], case["spacing"], case["dims"], **fc.ALL))):
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    out = _lib.FieldOut()
    d = np.zeros(2, np.float32)
    out.density = d.ctypes.data_as(C.POINTER(C.c_float))
    assert raw_call(w, 3, np.float32([[0, 0, 0], [1.0e9 * case["h"], 0, 0]]), out) == _lib.E_CAPACITY and "split the query" in last_error()


# 8 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [None, "64"])
def test_state(hip_lib, tmp_path, fold):
    """After 10 steps of a small dam break and after a host edit the evaluator sees the arrays get_fluid returns; a twin world that
    never evaluates has the same bits after 20 steps.  fold: the same with the step's grid folded (SALVA_HIP_FOLD_CELLS=64)."""
    s = child("state", tmp_path, **({"SALVA_HIP_FOLD_CELLS": fold} if fold else {}))
    assert np.array_equal(s["end_x"], s["twin_x"]) and np.array_equal(s["end_v"], s["twin_v"])
    n = len(s["a_x"])
    r = np.float32(0.05)  # basic3's particle radius; h as the library computes it (liquid_world.rs:44 in f32)
    h = float(np.float32(r * np.float32(2.0) * np.float32(2.0)))
    for tag in ("a", "b"):
        vol = s["a_vol"]
        ref = fr.evaluate(s["pts"], s[tag + "_x"], s[tag + "_v"], vol, np.full(n, 1000.0), h, border=1.0e-4 * float(r))
        assert ref["n"].max() > 20
        fr.compare({k: s[f"{tag}_{k}"] for k in fc.ALL}, ref)
    assert not np.array_equal(s["a_density"], s["b_density"])


# 9 ------------------------------------------------------------------------------------------------
def test_device_pointers(hip_lib, tmp_path):
    """Points and outputs in torch tensors on the device (data_ptr()), both flags: the bits are those of the host-pointer call.  In a
    child process, so that torch is loaded before the library (one HIP runtime per process)."""
    s = child("device", tmp_path)
    for where in ("points", "nodes"):
        for k in fc.ALL:
            dev, host = s[f"dev_{where}_{k}"], s[f"host_{where}_{k}"]
            assert np.array_equal(dev.view(host.dtype).reshape(host.shape), host), (where, k)
        assert s[f"host_{where}_count"].max() > 10


# 10 -----------------------------------------------------------------------------------------------
def test_refusals(hip_lib, case):
    from salva_amd import dist

    w, _ = fc.standard_world(case)
    pts = case["points"][:64].copy()
    pts[5, 1], pts[9, 0], pts[11, 2] = np.nan, np.inf, -np.inf
    got = fc.flat(w.evaluate_fields(pts, **fc.ALL))
    clean = fc.flat(w.evaluate_fields(case["points"][:64], **fc.ALL))
    for k in got:
        assert (got[k][[5, 9, 11]] == 0).all(), k
        keep = np.setdiff1d(np.arange(64), [5, 9, 11])
        assert np.array_equal(got[k][keep], clean[k][keep]), k
    allnan = fc.flat(w.evaluate_fields(np.full((7, 3), np.nan, np.float32), **fc.ALL))
    assert all((a == 0).all() for a in allnan.values())
    out = _lib.FieldOut()
    d = np.zeros(1 << 12, np.float32)
    out.density = d.ctypes.data_as(C.POINTER(C.c_float))
    assert raw_call(w, 3, pts, None) == _lib.E_INVALID
    assert raw_call(w, 3, pts, out, flags=4) == _lib.E_INVALID and "unknown flag" in last_error()
    assert w._L.salva_hip_evaluate_fields(w._h, 3, 0, None, 0, C.byref(out)) == _lib.OK  # npoints == 0: nothing to do
    o = case["origin"]
    for spacing in (0.0, -1.0, float("nan"), float("inf")):
        assert raw_lattice(w, 3, o, spacing, (2, 2, 2), out) == _lib.E_INVALID, spacing
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        assert raw_lattice(w, 3, o, 0.1, dims, out) == _lib.E_INVALID, dims
    assert raw_lattice(w, 3, o, 0.1, (2, 2, 2), None) == _lib.E_INVALID
    assert raw_lattice(w, 3, o, 0.1, (1 << 16, 1 << 16, 2), out) == _lib.E_CAPACITY and "2^32 nodes" in last_error()
    assert raw_lattice(w, 3, o, 1.0e6 * case["h"], (16, 16, 1), out) == _lib.E_CAPACITY and "split the query" in last_error()
    nan_origin = fc.flat(w.evaluate_lattice((np.nan, 0.0, 0.0), 0.1, (3, 3, 3), **fc.ALL))
    assert all((a == 0).all() for a in nan_origin.values())
    # a loopback-decomposed world
    wd, _ = fc.standard_world(case)
    comm = dist.Comm.loopback(1)[0]
    wd.set_domain(comm, -1000, 1000)
    assert raw_call(wd, 3, pts, out) == _lib.E_INVALID and "host-order arrays are not maintained" in last_error()
    assert raw_lattice(wd, 3, o, 0.1, (2, 2, 2), out) == _lib.E_INVALID and "host-order arrays are not maintained" in last_error()


def test_refused_inside_a_force_callback(hip_lib, case):
    from salva_amd import NonPressureForce

    class Calls(NonPressureForce):
        def solve(self, timestep, kernel_radius, ff, fb, fluid, boundaries, densities):
            out = _lib.FieldOut()
            d = np.zeros(8, np.float32)
            out.density = d.ctypes.data_as(C.POINTER(C.c_float))
            self.seen = (raw_call(self.world, 3, np.zeros((8, 3), np.float32), out), last_error(),
                         raw_lattice(self.world, 3, (0, 0, 0), 0.1, (2, 2, 2), out), last_error())

    w, (f0, _) = fc.standard_world(case)
    force = Calls()
    force.world = w
    f0.nonpressure_forces.append(force)
    st = w.step(fc.DT, (0.0, 0.0, 0.0))
    assert force.seen[0] == _lib.E_INVALID and force.seen[2] == _lib.E_INVALID and "callback" in force.seen[1] and "callback" in force.seen[3]
    assert st is not None and w._nsteps == 1  # the step completed


# 11 -----------------------------------------------------------------------------------------------
def test_mirrors(hip_lib, case):
    w, _ = fc.standard_world(case)
    got = w.evaluate_lattice(case["origin"], case["spacing"], case["dims"], **fc.ALL)
    nx, ny, nz = case["dims"]
    assert got["density"].shape == (nx, ny, nz) and got["fraction"].shape == (nx, ny, nz) and got["count"].shape == (nx, ny, nz)
    assert got["velocity"].shape == (nx, ny, nz, 3) and got["gradient"].shape == (nx, ny, nz, 3)
    assert got["count"].dtype == np.uint32 and got["density"].dtype == np.float32
    assert set(w.evaluate_fields(case["points"])) == {"density"}


def test_field_grid3_example_agrees_with_the_python_mirror(hip_lib):
    """examples/field_grid3.cpp: the basic3 block, 50 steps, the fraction on a lattice at spacing r; its printed node count is the
    Python mirror's on the same scene."""
    import re

    root = os.path.dirname(TESTS)
    exe = os.path.join(root, "examples", "field_grid3")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "examples"), "field_grid3"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"nodes above 0\.5: (\d+) of (\d+); fill height ([-0-9.eE+]+)", r.stdout)
    assert m, r.stdout
    above, total, height = fc.field_grid3()
    assert (int(m.group(1)), int(m.group(2))) == (above, total)
    assert abs(float(m.group(3)) - height) <= 1e-5
