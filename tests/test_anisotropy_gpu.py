"""The anisotropic kernels (include/salva_hip.h "Anisotropic kernels") on the device against the reading
tests/anisotropy_reading.py.  salva_hip_compute_anisotropy: `count` exactly, centres and h G within 4 x the distance between the reading
in f32 and in f64 on the same cloud (the device's Jacobi and its order of summation are not numpy's).  The evaluator: against the
reading fed the device's own centres and metrics, at the tolerance derived in the reading's docstring, with exact zeros where no
particle reaches.  Jobs that need a process of their own run as children (tests/anisotropy_child.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import anisotropy_child as ac
import anisotropy_reading as ar
import field_child as fc
import field_reading as fr
import surface_reading as sr
from salva_amd import _lib

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24
CANARY = 0x7FC0BEEF
DEFAULT = ar.Params()
LIMIT = ar.Params(lam=0.0, k_n=1.0, n_eps=ar.NEVER_ISOLATED_OFF)  # the isotropic limit


@pytest.fixture(scope="module")
def case():
    return ar.standard_cloud()


@pytest.fixture(scope="module")
def shapes():
    return ar.shapes_cloud()


@pytest.fixture(scope="module")
def world(hip_lib, case):
    return fc.standard_world(case)


@pytest.fixture(scope="module")
def rows(world):
    """the device's centres, metrics and counts of the standard cloud at the default parameters, shared and left unchanged"""
    return world[0].anisotropy(ac.mirror(DEFAULT))


def child(job, tmp_path):
    out = str(tmp_path / (job + ".npz"))
    e = dict(os.environ)
    for k in ("SALVA_HIP_FIELD_ARM", "SALVA_HIP_FOLD_CELLS", "SALVA_HIP_NO_FOLD"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(TESTS, "anisotropy_child.py"), job, out], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


def last_error():
    return _lib.lib().salva_hip_last_error().decode()


def f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def params(p=DEFAULT, **edit):
    s = ac.mirror(p)._struct()
    for k, v in edit.items():
        setattr(s, k, v)
    return s


def raw_points(w, mask, p, pts, out, flags=0):
    q = np.ascontiguousarray(pts, np.float32)
    return w._L.salva_hip_evaluate_fields_anisotropic(w._h, mask, C.byref(p) if p is not None else None, len(q), f32p(q), flags,
                                                      C.byref(out) if out is not None else None)


def raw_lattice(w, mask, p, origin, spacing, dims, out, flags=0):
    o, d = np.ascontiguousarray(origin, np.float32), np.ascontiguousarray(dims, np.uint32)
    return w._L.salva_hip_evaluate_fields_anisotropic_lattice(w._h, mask, C.byref(p) if p is not None else None, f32p(o), float(spacing), u32p(d), flags,
                                                              C.byref(out) if out is not None else None)


def raw_surface(w, mask, p, field, iso, origin, spacing, dims, out, counts, flags=0):
    o, d = np.ascontiguousarray(origin, np.float32), np.ascontiguousarray(dims, np.uint32)
    return w._L.salva_hip_extract_surface_anisotropic(w._h, mask, C.byref(p) if p is not None else None, field, float(iso), f32p(o), float(spacing),
                                                      u32p(d), flags, C.byref(out) if out is not None else None, counts)


def raw_compute(w, mask, p, out, nrows, flags=0):
    return w._L.salva_hip_compute_anisotropy(w._h, mask, C.byref(p) if p is not None else None, flags, C.byref(out) if out is not None else None,
                                             C.byref(nrows) if nrows is not None else None)


def check_rows(got, x, h, p):
    """compute_anisotropy's rows against the reading: counts exactly, the rest within 4 x the f32-f64 distance of the reading"""
    m64, m32 = ar.moments(x, h, p), ar.moments(x, h, p, dtype=np.float32)
    dc, dg = ar.distance(m32, m64, h)
    fin = m64["finite"]
    assert np.array_equal(got["count"].astype(np.int64), m64["count"])
    assert np.isfinite(got["metric"]).all() and np.isfinite(got["centres"][fin]).all()
    ec = float(np.abs(got["centres"].astype(np.float64) - m64["centres"])[fin].max()) / h
    eg = float(np.abs(got["metric"].astype(np.float64) - m64["metric"]).max()) * h
    print(f"centres / h: error {ec:.3e}, allowed 4 x {dc:.3e}; h G: error {eg:.3e}, allowed 4 x {dg:.3e}")
    assert ec <= 4.0 * dc and eg <= 4.0 * dg
    # a non-finite row: its position as it is, a zero metric, count 0
    bad = ~fin
    assert (got["metric"][bad] == 0.0).all() and (got["count"][bad] == 0).all()
    assert np.array_equal(got["centres"][bad].view(np.uint32), np.asarray(x, np.float32)[bad].view(np.uint32))
    return m64


# 1 ------------------------------------------------------------------------------------------------
def test_moments_of_the_standard_cloud(world, rows, case):
    w, _ = world
    check_rows(rows, case["x"], case["h"], DEFAULT)
    again = w.anisotropy(ac.mirror(DEFAULT))
    for k in rows:
        assert np.array_equal(rows[k].view(np.uint32), again[k].view(np.uint32)), k  # the order of every sum is fixed


@pytest.mark.parametrize("n_eps", [25, 4])
def test_moments_of_the_shapes(hip_lib, shapes, n_eps):
    p = ar.Params(n_eps=n_eps)
    w, _ = ac.one_fluid_world(shapes["x"], shapes["vol"], shapes["r"])
    got = w.anisotropy(ac.mirror(p))
    m = check_rows(got, shapes["x"], shapes["h"], p)
    parts = shapes["parts"]
    # C = 0 comes out finite and at the lower clamp; the isolated rows are I / (k_n h) exactly
    heap = got["metric"][parts["heap"]].astype(np.float64) * shapes["h"]
    assert np.abs(heap - np.array([4.0, 0, 0, 4.0, 0, 4.0])).max() <= 8.0 * U
    isolated = m["finite"] & (m["count"] <= n_eps)
    iso = got["metric"][isolated]
    assert (iso[:, [1, 2, 4]] == 0.0).all() and (iso[:, 0] == iso[:, 3]).all() and (iso[:, 0] == iso[:, 5]).all()
    assert np.abs(iso[:, 0].astype(np.float64) * (p.k_n * shapes["h"]) - 1.0).max() <= 4.0 * U  # (1 / h, then / k_n, and h itself is f32)


# 2 ------------------------------------------------------------------------------------------------
def masses(case):
    return case["vol"].astype(np.float64) * case["rho0"]


@pytest.mark.parametrize("kd,kg", fc.COMBOS)
def test_the_sums_on_the_points(hip_lib, case, kd, kg):
    """the reading is fed the device's own centres and metrics: only the sums are under test"""
    w, _ = fc.standard_world(case, kd, kg)
    prm = ac.mirror(DEFAULT)
    rows = w.anisotropy(prm)
    got = ac.flat(w.evaluate_fields(case["points"], anisotropy=prm, **ac.ALL))
    ref = ar.evaluate(case["points"], rows["centres"], rows["metric"], masses(case), case["vol"], fc.KINDS[kd], fc.KINDS[kg])
    assert ref["n"].max() > 20 and (ref["n"] == 0).any()
    ar.compare(got, ref)
    again = ac.flat(w.evaluate_fields(case["points"], anisotropy=prm, **ac.ALL))
    for k in got:
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), k


def coarse(case):
    """the standard box at spacing 2 r: 20 x 17 x 15 nodes"""
    dims = tuple((d + 1) // 2 for d in case["dims"])
    return case["origin"], np.float32(2.0 * case["r"]), dims


def test_the_sums_on_a_lattice(world, rows, case):
    w, _ = world
    origin, spacing, dims = coarse(case)
    got = w.evaluate_lattice(origin, spacing, dims, anisotropy=ac.mirror(DEFAULT), **ac.ALL)
    assert got["density"].shape == dims and got["gradient"].shape == dims + (3,) and got["density"].dtype == np.float32
    nodes = fr.lattice_nodes(origin, spacing, dims)
    ref = ar.evaluate(nodes, rows["centres"], rows["metric"], masses(case), case["vol"])
    ar.compare(ac.flat(got), ref)
    # the same nodes through the points entry: the same walk, the same bits
    pts = ac.flat(w.evaluate_fields(nodes, anisotropy=ac.mirror(DEFAULT), **ac.ALL))
    for k, v in ac.flat(got).items():
        assert np.array_equal(v.view(np.uint32), pts[k].view(np.uint32)), k


@pytest.mark.parametrize("n_eps", [25, 4])
def test_the_sums_around_the_shapes(hip_lib, shapes, n_eps):
    prm = ac.mirror(ar.Params(n_eps=n_eps))
    w, _ = ac.one_fluid_world(shapes["x"], shapes["vol"], shapes["r"])
    rows = w.anisotropy(prm)
    got = ac.flat(w.evaluate_fields(shapes["points"], anisotropy=prm, **ac.ALL))
    ref = ar.evaluate(shapes["points"], rows["centres"], rows["metric"], shapes["vol"].astype(np.float64) * shapes["rho0"], shapes["vol"])
    assert ref["n"].max() >= 30 and ref["n"][-2:].tolist() == [0, 0]
    ar.compare(got, ref)


def test_fluid_mask(world, case):
    w, (f0, f1) = world
    n0 = case["n0"]
    prm = ac.mirror(DEFAULT)
    for fluids, sl in (([f0], slice(0, n0)), ([1], slice(n0, None))):
        rows = w.anisotropy(prm, fluids=fluids)
        assert len(rows["count"]) == len(case["x"][sl])
        check_rows(rows, case["x"][sl], case["h"], DEFAULT)
        got = ac.flat(w.evaluate_fields(case["points"], fluids=fluids, anisotropy=prm, **ac.ALL))
        ar.compare(got, ar.evaluate(case["points"], rows["centres"], rows["metric"], masses(case)[sl], case["vol"][sl]))
    out = _lib.AnisoFieldOut()
    d = np.zeros(len(case["points"]), np.float32)
    out.density = f32p(d)
    assert raw_points(w, 0b100, params(), case["points"], out) == _lib.E_INVALID and "selects no existing fluid" in last_error()
    assert raw_points(w, 0b110, params(), case["points"], out) == _lib.OK  # (an absent fluid beside an existing one is ignored)
    assert np.array_equal(d, w.evaluate_fields(case["points"], fluids=[1], anisotropy=prm)["density"])


def test_output_subsets(world, case):
    w, _ = world
    pts, m = case["points"], len(case["points"])
    full = ac.flat(w.evaluate_fields(pts, anisotropy=ac.mirror(DEFAULT), **ac.ALL))
    widths = dict(density=1, fraction=1, gradient=3)
    for name in ac.ALL:
        bufs = {k: np.full(m * widths[k], CANARY, np.uint32) for k in ac.ALL}
        out = _lib.AnisoFieldOut()
        setattr(out, name, C.cast(u32p(bufs[name]), C.POINTER(C.c_float)))
        assert raw_points(w, 3, params(), pts, out) == _lib.OK, last_error()
        assert np.array_equal(bufs[name], full[name].reshape(-1).view(np.uint32)), name
        for k in ac.ALL:
            if k != name:
                assert (bufs[k] == CANARY).all(), (name, k)


def test_device_pointers(hip_lib, tmp_path):
    """Points, outputs and rows in torch tensors on the device: the bits of the host-pointer calls."""
    s = child("device", tmp_path)
    for where in ("points", "nodes"):
        for k in ac.ALL:
            dev, host = s[f"dev_{where}_{k}"], s[f"host_{where}_{k}"]
            assert np.array_equal(dev.view(np.uint32).reshape(-1), host.view(np.uint32).reshape(-1)), (where, k)
        assert s[f"host_{where}_density"].max() > 100.0
    for k in ("centres", "metric", "count"):
        assert np.array_equal(s["dev_" + k].view(np.uint32), s["host_" + k].view(np.uint32)), k
    assert int(s["nrows"][0]) == len(s["host_count"]) == 1386


# 3 ------------------------------------------------------------------------------------------------
def test_the_isotropic_limit(world, case):
    """n_eps = 2^32 - 1, k_n = 1, lambda = 0: G = I / h on the raw positions - salva_hip_evaluate_fields, within the two bounds added."""
    w, _ = world
    prm = ac.mirror(LIMIT)
    rows = w.anisotropy(prm)
    assert np.array_equal(rows["centres"].view(np.uint32), case["x"].view(np.uint32))
    got = ac.flat(w.evaluate_fields(case["points"], anisotropy=prm, density=True, gradient=True))
    iso = fc.flat(w.evaluate_fields(case["points"], density=True, gradient=True))
    a = ar.evaluate(case["points"], rows["centres"], rows["metric"], masses(case), case["vol"])
    b = fr.evaluate(case["points"], case["x"], case["v"], case["vol"], case["rho0"], case["h"])
    assert np.array_equal(a["n"], b["n"])
    for name, c in (("density", a["c_value"]), ("gradient", a["c_gradient"])):
        tol = ar.tol_sum(a["n"], a["A_" + name], c) + fr.tol_sum(b["n"], b["A_" + name])
        err = np.abs(got[name].astype(np.float64) - iso[name]).reshape(len(tol), -1)
        print(f"{name}: worst error / tolerance = {float((err[tol > 0] / tol[tol > 0, None]).max()):.4f}")
        assert (err <= tol[:, None]).all(), name
        assert (got[name][a["n"] == 0] == 0.0).all()


# 4 ------------------------------------------------------------------------------------------------
def same_mesh(got_v, got_t, ref_v, ref_t):
    assert got_t.shape == ref_t.shape and got_v.shape == ref_v.shape, (got_v.shape, got_t.shape, ref_v.shape, ref_t.shape)
    assert np.array_equal(got_t, ref_t)
    assert np.array_equal(np.ascontiguousarray(got_v).view(np.uint32), np.ascontiguousarray(ref_v).view(np.uint32))  # bit for bit


@pytest.mark.parametrize("field,iso", [("fraction", 0.5), ("density", 400.0)])
def test_the_surface_is_the_contour_of_the_lattice_call(world, case, field, iso):
    w, _ = world
    prm = ac.mirror(DEFAULT)
    origin, spacing, dims = case["origin"], case["spacing"], case["dims"]
    values = w.evaluate_lattice(origin, spacing, dims, anisotropy=prm, density=field == "density", fraction=field == "fraction")[field]
    want = w.extract_surface_from_values(values, origin, spacing, iso)
    mesh = w.extract_surface(origin, spacing, dims, iso=iso, field=field, anisotropy=prm, normals=True, velocities=True)
    assert len(mesh["vertices"]) > 1000
    same_mesh(mesh["vertices"], mesh["triangles"], want["vertices"], want["triangles"])
    ref_v, ref_t, _ = sr.extract(values, iso, origin, spacing)
    same_mesh(mesh["vertices"], mesh["triangles"], ref_v, ref_t)
    # normals: -g / |g| of the anisotropic gradient at the vertices (6 u: tests/test_surface_gpu.py); velocities: the isotropic evaluator's
    v, n = mesh["vertices"], mesh["normals"]
    g = w.evaluate_fields(v, anisotropy=prm, density=False, gradient=True)["gradient"].astype(np.float64)
    length = np.linalg.norm(g, axis=1)
    zero = length == 0.0
    assert (n[zero] == 0.0).all() and (~zero).mean() > 0.99
    err = np.abs(n[~zero].astype(np.float64) + g[~zero] / length[~zero, None]).max()
    print(f"worst normal component error: {err / U:.2f} u")
    assert err <= 6.0 * U
    vel = w.evaluate_fields(v, density=False, velocity=True)["velocity"]
    assert np.array_equal(mesh["velocities"].view(np.uint32), vel.view(np.uint32)) and np.abs(vel).max() > 0.1


def test_surface_counts_and_capacity(world, case):
    w, _ = world
    origin, spacing, dims = coarse(case)
    ref = w.extract_surface(origin, spacing, dims, anisotropy=ac.mirror(DEFAULT))
    nv, nt = len(ref["vertices"]), len(ref["triangles"])
    assert nv > 100
    counts = (C.c_uint64 * 2)()
    assert raw_surface(w, 3, params(), _lib.SURFACE_FRACTION, 0.5, origin, spacing, dims, None, counts) == _lib.OK and (counts[0], counts[1]) == (nv, nt)
    for vcap, tcap, code in ((nv - 1, nt, _lib.E_CAPACITY), (nv, nt - 1, _lib.E_CAPACITY), (nv, nt, _lib.OK)):
        bufs = {"vertices": np.full(3 * nv + 3, CANARY, np.uint32), "triangles": np.full(3 * nt + 3, CANARY, np.uint32)}
        out = _lib.SurfaceOut()
        out.vertices, out.triangles = C.cast(u32p(bufs["vertices"]), C.POINTER(C.c_float)), u32p(bufs["triangles"])
        out.vertex_capacity, out.triangle_capacity = vcap, tcap
        counts = (C.c_uint64 * 2)()
        assert raw_surface(w, 3, params(), _lib.SURFACE_FRACTION, 0.5, origin, spacing, dims, out, counts) == code, last_error()
        assert (counts[0], counts[1]) == (nv, nt)
        if code != _lib.OK:
            assert all((b == CANARY).all() for b in bufs.values())
        else:
            same_mesh(bufs["vertices"][:3 * nv].view(np.float32).reshape(nv, 3), bufs["triangles"][:3 * nt].reshape(nt, 3), ref["vertices"], ref["triangles"])
            assert (bufs["vertices"][3 * nv:] == CANARY).all() and (bufs["triangles"][3 * nt:] == CANARY).all()


def test_rows_counts_and_capacity(world, rows, case):
    w, _ = world
    n = len(case["x"])
    nrows = C.c_uint64(0)
    assert raw_compute(w, 3, params(), None, nrows) == _lib.OK and nrows.value == n  # count only
    bufs = {"centres": np.full(3 * n + 3, CANARY, np.uint32), "metric": np.full(6 * n + 6, CANARY, np.uint32), "count": np.full(n + 1, CANARY, np.uint32)}
    out = _lib.AnisotropyOut()
    out.centres, out.metric = C.cast(u32p(bufs["centres"]), C.POINTER(C.c_float)), C.cast(u32p(bufs["metric"]), C.POINTER(C.c_float))
    out.count = u32p(bufs["count"])
    out.row_capacity = n - 1
    nrows = C.c_uint64(0)
    assert raw_compute(w, 3, params(), out, nrows) == _lib.E_CAPACITY and nrows.value == n, last_error()
    assert all((b == CANARY).all() for b in bufs.values())
    out.row_capacity = n
    assert raw_compute(w, 3, params(), out, nrows) == _lib.OK, last_error()
    for k, width in (("centres", 3), ("metric", 6), ("count", 1)):
        assert np.array_equal(bufs[k][:width * n], rows[k].reshape(-1).view(np.uint32)), k
        assert (bufs[k][width * n:] == CANARY).all(), k
    # a subset of the outputs
    only = _lib.AnisotropyOut()
    c = np.full(n, CANARY, np.uint32)
    only.count, only.row_capacity = u32p(c), n
    assert raw_compute(w, 3, params(), only, nrows) == _lib.OK and np.array_equal(c, rows["count"])


# 5 ------------------------------------------------------------------------------------------------
def test_the_anisotropic_surface_of_a_block_at_rest_is_flatter(hip_lib):
    """The top face of a jittered block at rest, `fraction` = 0.5, the same lattice: the vertex heights scatter strictly less with the
    default anisotropic kernels than with the isotropic extraction (tests/test_anisotropy_cpu.py shows it on the reading)."""
    b = ar.rest_block()
    w, _ = ac.one_fluid_world(b["x"], b["vol"], b["r"], density0=1000.0)
    iso = w.extract_surface(b["origin"], b["spacing"], b["dims"])
    aniso = w.extract_surface(b["origin"], b["spacing"], b["dims"], anisotropy=ac.mirror(DEFAULT))
    spread = {k: float(ar.top_heights(m["vertices"]).std()) / b["r"] for k, m in (("isotropic", iso), ("anisotropic", aniso))}
    print("standard deviation of the top face's vertex heights, in r:", spread)
    assert len(iso["vertices"]) > 500 and len(aniso["vertices"]) > 500
    assert spread["anisotropic"] < spread["isotropic"]


# 6 ------------------------------------------------------------------------------------------------
def test_state(hip_lib, tmp_path):
    """A twin world that never calls has the same bits after 20 steps; a second call gives the same bits; the calls see the arrays
    get_fluid returns."""
    s = child("state", tmp_path)
    assert np.array_equal(s["end_x"], s["twin_x"]) and np.array_equal(s["end_v"], s["twin_v"])
    for k in ("centres", "metric", "count", "vertices", "triangles", "normals", "lattice"):
        assert np.array_equal(s["a_" + k].view(np.uint32), s["b_" + k].view(np.uint32)), k
    h = float(np.float32(np.float32(0.05) * np.float32(2.0) * np.float32(2.0)))
    # (a simulated cloud is not separated: the rows with a pair on the border of 2h are left out of the exact comparison)
    m = ar.moments(s["x"], h)
    keep = np.setdiff1d(np.arange(len(m["count"])), np.unique(ar.near_the_border(s["x"], h)))
    assert len(keep) > 0.9 * len(m["count"])
    assert np.array_equal(s["a_count"].astype(np.int64)[keep], m["count"][keep])
    assert len(s["a_vertices"]) > 500 and s["a_count"].max() > 100


def test_strays_change_nothing(hip_lib, case):
    far = np.float32([[1.0e6 * case["h"], 0.0, 0.0], [0.1, -1.0e6 * case["h"], 0.2]])
    w, _ = fc.standard_world(case)
    ws, _ = fc.standard_world(case, extra=far)
    prm = ac.mirror(DEFAULT)
    origin, spacing, dims = coarse(case)
    for a, b in ((w.evaluate_fields(case["points"], anisotropy=prm, **ac.ALL), ws.evaluate_fields(case["points"], anisotropy=prm, **ac.ALL)),
                 (w.evaluate_lattice(origin, spacing, dims, anisotropy=prm, **ac.ALL), ws.evaluate_lattice(origin, spacing, dims, anisotropy=prm, **ac.ALL))):
        for k in a:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    # the table over the fluids' own box is another matter
    nrows = C.c_uint64(0)
    out = _lib.AnisotropyOut()
    c = np.zeros(len(case["x"]) + 2, np.uint32)
    out.count, out.row_capacity = u32p(c), len(c)
    ws.sync_to_device(apply_removal=False)
    assert raw_compute(ws, 3, params(), out, nrows) == _lib.E_CAPACITY and "2^27 cells" in last_error()


def test_refusals_and_edge_cases(hip_lib, case):
    from salva_amd import dist

    w, _ = fc.standard_world(case)
    w.sync_to_device(apply_removal=False)
    pts = case["points"][:64].copy()
    d = np.zeros(1 << 12, np.float32)
    out = _lib.AnisoFieldOut()
    out.density = f32p(d)
    nrows = C.c_uint64(0)
    counts = (C.c_uint64 * 2)()
    o = case["origin"]

    def refused(code, want=_lib.E_INVALID, text=None):
        assert code == want, (code, last_error())
        if text:
            assert text in last_error(), last_error()
        w.step(fc.DT, (0.0, 0.0, 0.0))  # the world steps on after every refusal

    nan = float("nan")
    for edit in (dict(lam=-0.1), dict(lam=1.5), dict(lam=nan), dict(k_r=0.5), dict(k_r=nan), dict(k_r=float("inf")), dict(k_s=0.0), dict(k_s=-1.0),
                 dict(k_s=float("inf")), dict(k_s=nan), dict(k_n=0.2), dict(k_n=2.5), dict(k_n=nan), dict(struct_size=60), dict(version=2)):
        refused(raw_points(w, 3, params(**edit), pts, out))
        assert raw_compute(w, 3, params(**edit), None, nrows) == _lib.E_INVALID, edit
        assert raw_lattice(w, 3, params(**edit), o, 0.1, (2, 2, 2), out) == _lib.E_INVALID, edit
        assert raw_surface(w, 3, params(**edit), _lib.SURFACE_FRACTION, 0.5, o, 0.1, (2, 2, 2), None, counts) == _lib.E_INVALID, edit
    refused(raw_points(w, 3, None, pts, out))
    refused(raw_points(w, 3, params(), pts, None))
    refused(raw_points(w, 3, params(), pts, out, flags=4), text="unknown flag")
    refused(raw_compute(w, 3, params(), None, nrows, flags=2), text="unknown flag")
    refused(raw_compute(w, 3, params(), None, None))
    refused(raw_surface(w, 3, params(), _lib.SURFACE_FRACTION, 0.5, o, 0.1, (2, 2, 2), None, counts, flags=1), text="unknown flag")
    refused(raw_surface(w, 3, params(), 7, 0.5, o, 0.1, (2, 2, 2), None, counts), text="unknown field")
    refused(raw_surface(w, 3, params(), _lib.SURFACE_FRACTION, nan, o, 0.1, (2, 2, 2), None, counts))
    refused(raw_surface(w, 3, params(), _lib.SURFACE_FRACTION, 0.5, o, 0.1, (1, 2, 2), None, counts))
    for spacing in (0.0, -1.0, nan, float("inf")):
        refused(raw_lattice(w, 3, params(), o, spacing, (2, 2, 2), out))
    refused(raw_lattice(w, 3, params(), o, 0.1, (0, 2, 2), out))
    refused(raw_lattice(w, 3, params(), o, 0.1, (1 << 16, 1 << 16, 2), out), _lib.E_CAPACITY, "2^32 nodes")
    refused(raw_lattice(w, 3, params(), o, 1.0e6 * case["h"], (16, 16, 1), out), _lib.E_CAPACITY, "split the query")
    refused(raw_points(w, 3, params(), np.float32([[0, 0, 0], [1.0e9 * case["h"], 0, 0]]), out), _lib.E_CAPACITY, "split the query")
    # edge cases that are no errors
    assert w._L.salva_hip_evaluate_fields_anisotropic(w._h, 3, C.byref(params()), 0, None, 0, C.byref(out)) == _lib.OK  # npoints == 0
    prm = ac.mirror(DEFAULT)
    bad = pts.copy()
    bad[5, 1], bad[9, 0], bad[11, 2] = np.nan, np.inf, -np.inf
    got, clean = ac.flat(w.evaluate_fields(bad, anisotropy=prm, **ac.ALL)), ac.flat(w.evaluate_fields(pts, anisotropy=prm, **ac.ALL))
    keep = np.setdiff1d(np.arange(64), [5, 9, 11])
    for k in got:
        assert (got[k][[5, 9, 11]] == 0).all() and np.array_equal(got[k][keep], clean[k][keep]), k
    assert all((a == 0).all() for a in w.evaluate_fields(np.full((7, 3), np.nan, np.float32), anisotropy=prm, **ac.ALL).values())
    assert all((a == 0).all() for a in w.evaluate_lattice((np.nan, 0.0, 0.0), 0.1, (3, 3, 3), anisotropy=prm, **ac.ALL).values())
    with pytest.raises(ValueError):
        w.evaluate_fields(pts, anisotropy=prm, velocity=True)
    # a loopback-decomposed world
    wd, _ = fc.standard_world(case)
    wd.sync_to_device(apply_removal=False)
    wd.set_domain(dist.Comm.loopback(1)[0], -1000, 1000)
    for code in (raw_points(wd, 3, params(), pts, out), raw_lattice(wd, 3, params(), o, 0.1, (2, 2, 2), out), raw_compute(wd, 3, params(), None, nrows),
                 raw_surface(wd, 3, params(), _lib.SURFACE_FRACTION, 0.5, o, 0.1, (2, 2, 2), None, counts)):
        assert code == _lib.E_INVALID and "host-order arrays are not maintained" in last_error()


def test_mirrors(world, case):
    w, _ = world
    from salva_amd import Anisotropy

    rows = w.anisotropy()  # the default parameters
    n = len(case["x"])
    assert rows["centres"].shape == (n, 3) and rows["metric"].shape == (n, 6) and rows["count"].shape == (n,)
    assert rows["centres"].dtype == np.float32 and rows["count"].dtype == np.uint32
    assert np.array_equal(rows["metric"], w.anisotropy(Anisotropy())["metric"])
    assert set(w.evaluate_fields(case["points"], anisotropy=Anisotropy())) == {"density"}
    assert w.evaluate_fields(case["points"], anisotropy=Anisotropy(), density=False, gradient=True)["gradient"].shape == (len(case["points"]), 3)


def test_anisotropic_surface3_example_agrees_with_the_python_mirror(hip_lib, tmp_path):
    """examples/anisotropic_surface3.cpp: the basic3 block after 50 steps, both surfaces with normals: its counts and its two OBJ files are
    the Python mirror's meshes of the same scene."""
    import re

    root = os.path.dirname(TESTS)
    exe = os.path.join(root, "examples", "anisotropic_surface3")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "examples"), "anisotropic_surface3"], stdout=subprocess.DEVNULL)
    prefix = str(tmp_path / "mesh")
    r = subprocess.run([exe, prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for name, mesh in zip(("isotropic", "anisotropic"), ac.anisotropic_surface3()):
        m = re.search(name + r": vertices: (\d+); triangles: (\d+); volume ([-0-9.eE+]+); area ([-0-9.eE+]+)", r.stdout)
        assert m, r.stdout
        v, t, n = mesh["vertices"], mesh["triangles"], mesh["normals"]
        assert (int(m.group(1)), int(m.group(2))) == (len(v), len(t)) and len(v) > 1000
        assert abs(float(m.group(3)) - sr.signed_volume(v, t)) <= 1e-5 and abs(float(m.group(4)) - sr.area(v, t)) <= 1e-4
        lines = open(f"{prefix}_{name}.obj").read().split("\n")
        got_v = np.array([ln.split()[1:] for ln in lines if ln.startswith("v ")], np.float32)
        got_n = np.array([ln.split()[1:] for ln in lines if ln.startswith("vn ")], np.float32)
        got_f = np.array([[int(c.split("//")[0]) for c in ln.split()[1:]] for ln in lines if ln.startswith("f ")], np.int64)
        assert np.array_equal(got_v, v) and np.array_equal(got_n, n)  # (printed with nine significant digits: f32 round trip)
        assert np.array_equal(got_f - 1, t.astype(np.int64))
        unique, open_edges = sr.edge_report(t)
        assert unique and len(open_edges) == 0  # (the lattice encloses what the kernels reach: a closed mesh)


def test_refused_inside_a_force_callback(hip_lib, case):
    from salva_amd import NonPressureForce

    class Calls(NonPressureForce):
        def solve(self, timestep, kernel_radius, ff, fb, fluid, boundaries, densities):
            out = _lib.AnisoFieldOut()
            d = np.zeros(8, np.float32)
            out.density = f32p(d)
            nrows, counts = C.c_uint64(0), (C.c_uint64 * 2)()
            self.seen = [(raw_points(self.world, 3, params(), np.zeros((8, 3), np.float32), out), last_error()),
                         (raw_lattice(self.world, 3, params(), (0, 0, 0), 0.1, (2, 2, 2), out), last_error()),
                         (raw_compute(self.world, 3, params(), None, nrows), last_error()),
                         (raw_surface(self.world, 3, params(), _lib.SURFACE_FRACTION, 0.5, (0, 0, 0), 0.1, (2, 2, 2), None, counts), last_error())]

    w, (f0, _) = fc.standard_world(case)
    force = Calls()
    force.world = w
    f0.nonpressure_forces.append(force)
    st = w.step(fc.DT, (0.0, 0.0, 0.0))
    assert all(code == _lib.E_INVALID and "callback" in text for code, text in force.seen), force.seen
    assert st is not None and w._nsteps == 1  # the step completed
