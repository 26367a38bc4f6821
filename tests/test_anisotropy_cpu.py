"""The anisotropic kernels (include/salva_hip.h "Anisotropic kernels") without a GPU: the invariants of the reading
tests/anisotropy_reading.py, the conditions the inputs of tests/test_anisotropy_gpu.py must meet, the f32-against-f64 distance of the
reading that the GPU test's tolerance is made from, the inequality the whole feature is for, and the library's new symbols."""
import ctypes as C

import numpy as np
import pytest

import anisotropy_reading as ar
import field_reading as fr
import surface_reading as sr

NEW_SYMBOLS = ("salva_hip_default_anisotropy", "salva_hip_compute_anisotropy", "salva_hip_evaluate_fields_anisotropic",
               "salva_hip_evaluate_fields_anisotropic_lattice", "salva_hip_extract_surface_anisotropic")


@pytest.fixture(scope="module")
def standard():
    return ar.standard_cloud()


@pytest.fixture(scope="module")
def shapes():
    return ar.shapes_cloud()


@pytest.fixture(scope="module")
def readings(standard, shapes):
    """(cloud, parameters) -> the reading in f64 and in f32, computed once"""
    out = {}
    for name, x, h, p in (("standard", standard["x"], standard["h"], ar.Params()), ("shapes", shapes["x"], shapes["h"], ar.Params()),
                          ("shapes4", shapes["x"], shapes["h"], ar.Params(n_eps=4))):
        out[name] = (ar.moments(x, h, p), ar.moments(x, h, p, dtype=np.float32), h, p)
    return out


def test_the_library_exports_the_new_entry_points(hip_lib):
    from salva_amd import _lib

    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name), name
    assert C.sizeof(_lib.AnisotropyParams) == _lib.ANISOTROPY_BYTES == 64
    p = _lib.AnisotropyParams()
    hip_lib.salva_hip_default_anisotropy(C.byref(p))
    d = ar.Params()
    assert (p.struct_size, p.version, p.n_eps) == (64, 1, d.n_eps)
    assert (p.lam, p.k_r, p.k_s, p.k_n) == tuple(float(np.float32(v)) for v in (d.lam, d.k_r, d.k_s, d.k_n))
    assert all(v == 0 for v in p.reserved)
    from salva_amd import Anisotropy

    q = Anisotropy()._struct()
    assert bytes(q) == bytes(p)


@pytest.mark.parametrize("name", ["standard", "shapes", "shapes4"])
def test_the_metric_is_positive_definite_and_bounded(readings, standard, shapes, name):
    m, _, h, p = readings[name]
    cloud = (standard if name == "standard" else shapes)["x"].astype(np.float64)
    fin = m["finite"]
    eig = np.linalg.eigvalsh(ar.full(m["metric"][fin]))
    assert (eig >= (1.0 - 1e-12) / (ar.S_HI * h)).all() and (eig <= (1.0 + 1e-12) / (ar.S_LO * h)).all()
    isolated = fin & (m["count"] <= p.n_eps)
    assert isolated.any() == (name != "standard")
    want = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0]) / (p.k_n * h)
    assert (m["metric"][isolated] == want).all()  # exactly
    assert (m["metric"][~fin] == 0.0).all() and (m["count"][~fin] == 0).all()
    # the centre stays within lambda * 2h of its particle
    assert (np.linalg.norm(m["centres"][fin] - cloud[fin], axis=1) <= p.lam * 2.0 * h * (1.0 + 1e-12)).all()


def test_the_isotropic_limit_is_the_field_evaluator(standard):
    p = ar.Params(lam=0.0, k_n=1.0, n_eps=ar.NEVER_ISOLATED_OFF)
    m = ar.moments(standard["x"], standard["h"], p)
    assert np.array_equal(m["centres"], standard["x"].astype(np.float64))
    pts = standard["points"][:600]
    mass = standard["vol"].astype(np.float64) * standard["rho0"]
    for kd, kg in ((fr.CUBIC, fr.CUBIC), (fr.POLY6, fr.SPIKY), (fr.VISCOSITY, fr.VISCOSITY)):
        a = ar.evaluate(pts, m["centres"], m["metric"], mass, standard["vol"], kd, kg)
        b = fr.evaluate(pts, standard["x"], standard["v"], standard["vol"], standard["rho0"], standard["h"], kd, kg)
        assert np.array_equal(a["n"], b["n"]) and a["n"].max() > 20
        for k in ("density", "fraction", "gradient"):
            scale = np.abs(b[k]).max()
            assert np.abs(a[k] - b[k]).max() <= 1e-11 * scale, (kd, kg, k)


def test_the_inputs_meet_their_conditions(standard, shapes, readings):
    """No pair within 1e-4 h of 2h (so that `count` can be compared exactly on every row), and every shape is what it is there for."""
    assert len(ar.near_the_border(standard["x"], standard["h"])) == 0
    assert len(ar.near_the_border(shapes["x"], shapes["h"])) == 0
    assert len(ar.near_the_border(ar.rest_block()["x"], fr.H32)) == 0
    for name in ("standard", "shapes", "shapes4"):
        m64, m32, _, _ = readings[name]
        assert np.array_equal(m64["count"], m32["count"]), name
    assert len(standard["x"]) == 1386
    # (a): no clamp is active in the standard case
    s = readings["standard"][0]["s"]
    assert s.min() > ar.S_LO and s.max() < ar.S_HI and readings["standard"][0]["count"].min() > 25
    parts = shapes["parts"]
    m, m4 = readings["shapes"][0], readings["shapes4"][0]
    assert m["count"][parts["block"]].max() > 200
    # the sheet: the smallest stretch is the largest over k_r, or S_LO
    sh = m["s"][parts["sheet"]][m["count"][parts["sheet"]] > 25]
    assert len(sh) and np.allclose(sh[:, 2], np.maximum(sh[:, 0] / 4.0, ar.S_LO), rtol=1e-12)
    # the line: isolated at n_eps = 25, two equal small eigenvalues at n_eps = 4
    assert (m["count"][parts["line"]] <= 25).all() and (m4["count"][parts["line"]] > 4).sum() >= 10
    ln = m4["s"][parts["line"]][m4["count"][parts["line"]] > 4]
    assert (ln[:, 1] == ln[:, 2]).all() and (ln[:, 0] > ln[:, 1]).all()
    assert (m["count"][parts["pair"]] == 1).all() and (m["count"][parts["lone"]] == 0).all() and (m["count"][parts["stray"]] == 0).all()
    assert (m["count"][parts["heap"]] == 29).all() and (m["s"][parts["heap"]] == ar.S_LO).all()  # C = 0
    assert not m["finite"][parts["nan"]].any() and np.isnan(m["centres"][parts["nan"]]).any()


def test_the_distance_between_the_reading_in_f32_and_in_f64(readings):
    """What tests/test_anisotropy_gpu.py multiplies by 4 (DESIGN.md §23 records the figures)."""
    for name, (m64, m32, h, _) in readings.items():
        dc, dg = ar.distance(m32, m64, h)
        print(f"{name}: centres / h {dc:.3e}, h G {dg:.3e}")
        assert 0.0 < dc < 1e-4 and 0.0 < dg < 1e-4


def test_parameter_ranges():
    assert ar.valid(ar.Params())
    for bad in (ar.Params(lam=-0.1), ar.Params(lam=1.1), ar.Params(lam=float("nan")), ar.Params(k_r=0.5), ar.Params(k_r=float("inf")),
                ar.Params(k_s=0.0), ar.Params(k_s=float("inf")), ar.Params(k_n=0.2), ar.Params(k_n=2.5), ar.Params(k_n=float("nan"))):
        assert not ar.valid(bad), bad


def test_the_anisotropic_surface_of_a_block_at_rest_is_flatter():
    """The top face of a jittered block at rest, `fraction` = 0.5 on the same lattice: the vertex heights of the anisotropic surface
    (default parameters) scatter strictly less than those of the isotropic one - on the reading; the GPU test asserts it on the device."""
    b = ar.rest_block()
    x, n = b["x"], len(b["x"])
    vol = np.full(n, b["vol"], np.float32)
    nodes = fr.lattice_nodes(b["origin"], b["spacing"], b["dims"])
    iso = fr.evaluate(nodes, x, np.zeros_like(x), vol, np.full(n, 1000.0), b["h"])["fraction"]
    m = ar.moments(x, b["h"])
    aniso = ar.evaluate(nodes, m["centres"], m["metric"], vol.astype(np.float64) * 1000.0, vol)["fraction"]
    spread = {}
    for name, f in (("isotropic", iso), ("anisotropic", aniso)):
        v, _, _ = sr.extract(f.reshape(b["dims"]).astype(np.float32), 0.5, b["origin"], b["spacing"])
        assert len(v) > 500
        spread[name] = float(ar.top_heights(v).std()) / b["r"]
    print("standard deviation of the top face's vertex heights, in r:", spread)
    assert spread["anisotropic"] < spread["isotropic"]
