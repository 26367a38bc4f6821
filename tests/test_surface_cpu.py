"""The surface extractor's reading (tests/surface_reading.py) checked without a GPU: on a random lattice every case of the six
tetrahedra occurs and the mesh is a manifold that is open only on the lattice box; on a linear field the vertices lie on the plane at
a derived bound and every triangle faces down the gradient; on the standard case of the field evaluator the surfaces of
fraction = 0.5 and density = 400 are closed, of genus 0 and enclose about the fluid's volume.  And the library exports the entry
points."""
import numpy as np
import pytest

import field_reading as fr
import surface_reading as sr

U = 2.0 ** -24


def test_random_lattice_covers_every_case_and_is_a_manifold():
    f = sr.random_lattice()
    v, t, seen = sr.extract(f, 0.5, sr.LATTICE_ORIGIN, sr.LATTICE_SPACING)
    assert len(seen) == 84 and seen == {(k, m) for k in range(6) for m in range(1, 15)}  # a condition of the GPU tests
    assert len(v) and len(t) and t.dtype == np.uint32 and v.dtype == np.float32
    assert np.array_equal(np.unique(t), np.arange(len(v)))  # every vertex is referenced
    unique, open_edges = sr.edge_report(t)
    assert unique  # no directed edge occurs twice
    # an edge without its reverse has both ends on one face of the lattice box
    lo = np.array([sr.axis_nodes(sr.LATTICE_ORIGIN[a], sr.LATTICE_SPACING, d)[0] for a, d in enumerate(f.shape)])
    hi = np.array([sr.axis_nodes(sr.LATTICE_ORIGIN[a], sr.LATTICE_SPACING, d)[-1] for a, d in enumerate(f.shape)])
    assert len(open_edges)
    a, b = v[open_edges[:, 0]], v[open_edges[:, 1]]
    on_one_face = np.zeros(len(open_edges), bool)
    for k in range(3):
        for wall in (lo[k], hi[k]):
            on_one_face |= (a[:, k] == wall) & (b[:, k] == wall)
    assert on_one_face.all()


def test_linear_field_vertices_lie_on_the_plane():
    """With L(x) = n . x, M = sum_a |n_a| max |x_a| >= |L| on the lattice and u = 2^-24: the node values are L rounded once, so the
    exact interpolation x* of the exact t* between two of them has |L(x*) - iso| <= u M.  The computed t carries three roundings
    (numerator, denominator, quotient), Pb - Pa one, the product one: 5 u t |Pb - Pa| <= 5 u max |x_a| per axis (the spacing is below
    every max |x_a| here), and the final sum one more, u |x_a|.  Together |L(x) - iso| <= (1 + 5 + 1) u M: k = 7, and the |iso| of the
    bound's form is slack."""
    f = sr.linear_lattice()
    n = np.array(sr.LINEAR_N)
    iso = np.float32(sr.LINEAR_ISO)
    v, t, _ = sr.extract(f, iso, sr.LATTICE_ORIGIN, sr.LATTICE_SPACING)
    assert len(t) > 20
    x = v.astype(np.float64)
    bound = 7.0 * U * (float(np.abs(n) @ np.abs(x).max(axis=0)) + abs(float(iso)))
    err = np.abs(x @ n - float(iso)).max()
    print(f"worst |n . x - iso| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    p = x[t.astype(np.int64)]
    normals = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert ((normals @ n) < 0.0).all()  # towards lower values


@pytest.fixture(scope="module")
def standard_fields():
    c = fr.standard_case()
    ref = fr.evaluate(c["nodes"], c["x"], c["v"], c["vol"], c["rho0"], c["h"])
    return c, {k: ref[k].reshape(c["dims"]).astype(np.float32) for k in ("fraction", "density")}


@pytest.mark.parametrize("field,iso", [("fraction", 0.5), ("density", 400.0)])
def test_standard_case_surface_is_closed(standard_fields, field, iso):
    c, fields = standard_fields
    assert c["dims"] == (39, 33, 29)
    v, t, _ = sr.extract(fields[field], iso, c["origin"], c["spacing"])
    unique, open_edges = sr.edge_report(t)
    assert unique and len(open_edges) == 0  # every directed edge once, its reverse present
    assert sr.euler_characteristic(len(v), t) == 2
    volume = sr.signed_volume(v, t)
    total, block = float(c["vol"].astype(np.float64).sum()), float(np.prod(fr.GRID)) * (2.0 * fr.R) ** 3
    print(f"{field}: {len(v)} vertices, {len(t)} triangles, volume {volume:.4f} (sum V_j {total:.4f}, block {block:.4f})")
    assert 0.9 * total < volume < block


def test_exported_symbols():
    from salva_amd import _lib

    for name in ("salva_hip_extract_surface", "salva_hip_extract_surface_from_values", "salva_hip_get_fluid_bounds"):
        assert name in _lib.EXPORTED_SYMBOLS
    out = _lib.SurfaceOut()
    assert [f[0] for f in out._fields_] == ["vertices", "normals", "velocities", "triangles", "vertex_capacity", "triangle_capacity"]
