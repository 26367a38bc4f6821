"""The mesh readings (tests/mesh_reading.py) against things known without them, no GPU: the cube's volume samples
against the closed-form cuboid, the projection against an f64 brute force, inside / outside on the cube, and the height field's
vertex and triangle formulas on a case written out by hand."""
import numpy as np

import mesh_fixtures as X
import mesh_reading as M
import sampling_reading as R

F = np.float32


def test_cube_volume_samples_equal_the_cuboids():
    """r = 1 / 16: the lattice is dyadic, every operation exact, and the lattice lines with c_j == c_k run exactly through each face's
    diagonal — inclusive edges plus the s / 10 rule neither leak nor count twice."""
    v, t, _ = X.cube()
    hits = []
    q, pos, N = M.sample_mesh(v, t, 0.0625, R.VOLUME, hits)
    qc, posc, Nc = R.sample(("cuboid", (0.5, 0.5, 0.5)), 0.0625, R.VOLUME)
    assert N == Nc and len(pos) > 0
    assert {tuple(r) for r in q} == {tuple(r) for r in qc}
    assert np.array_equal(pos, posc)
    assert set(hits) == {0, 2}, "a ray through the cube has exactly one entry and one exit"


def test_l_prism_has_rays_with_two_intervals():
    v, t, _ = X.l_prism()
    hits = []
    M.sample_mesh(v, t, 0.02, R.VOLUME, hits)
    # (a chord shorter than s / 10 near a corner has its entry only: odd counts are the thin-chord rule, not a leak)
    assert max(hits) == 4 and hits.count(4) > 10


def _brute64(v, t, p):
    """f64 closest distance of every point to every triangle (Ericson's walk again, in f64) -> (n,) minimum."""
    v64 = np.asarray(v, np.float64)
    best = np.full(len(p), np.inf)
    for tri in np.asarray(t, np.int64):
        a, b, c = v64[tri]
        for r, x in enumerate(np.asarray(p, np.float64)):
            ab, ac, ap = b - a, c - a, x - a
            d1, d2 = ab @ ap, ac @ ap
            bp = x - b
            d3, d4 = ab @ bp, ac @ bp
            cp = x - c
            d5, d6 = ab @ cp, ac @ cp
            vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
            if d1 <= 0 and d2 <= 0:
                y = a
            elif d3 >= 0 and d4 <= d3:
                y = b
            elif vc <= 0 and d1 >= 0 and d3 <= 0:
                y = a + ab * (d1 / (d1 - d3))
            elif d6 >= 0 and d5 <= d6:
                y = c
            elif vb <= 0 and d2 >= 0 and d6 <= 0:
                y = a + ac * (d2 / (d2 - d6))
            elif va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
                y = b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))
            else:
                y = a + ab * (vb / (va + vb + vc)) + ac * (vc / (va + vb + vc))
            best[r] = min(best[r], np.linalg.norm(x - y))
    return best


def test_projection_agrees_with_an_f64_brute_force():
    """2 000 seeded points around (a), (b) and (e).  Compared are DISTANCES (the closest point itself jumps across a medial
    surface): |p - proj| against the f64 minimum, and the f64 distance of proj to the mesh.  Tolerance: the f32 walk forms its
    barycentric coordinates from differences of products of four lengths <= L = |p| + |v| <= 2.5, each product rounded to
    2^-24 L^4, divided by (twice the triangle's area)^2 >= 0.04 here: 2^-24 * 2.5^4 / 0.04 * 8 operations ~ 5e-4 relative on the
    coordinate in the worst corner, which moves the point along the triangle, not away from p; the distance changes by the
    square of that times the edge length plus the plain rounding of the coordinates, 2^-24 * L per operation.  16 roundings of
    2^-24 * 2.5 = 2.4e-6 bound it."""
    rng = np.random.default_rng(7)
    for fixture in (X.cube, X.l_prism, X.tetrahedron):
        v, t, _ = fixture()
        lo, hi = M.mesh_aabb(v)
        p = (lo - 0.4 + rng.random((2000, 3)) * (hi - lo + 0.8)).astype(F)
        proj, _ = M.mesh_project(v, t, None, p)
        d32 = np.linalg.norm(p.astype(np.float64) - proj.astype(np.float64), axis=1)
        d64 = _brute64(v, t, p)
        tol = 16 * 2.0 ** -24 * 2.5
        print(fixture.__name__, "max |d32 - d64| =", np.abs(d32 - d64).max(), "tol", tol)
        assert np.abs(d32 - d64).max() <= tol
        assert _brute64(v, t, proj).max() <= tol


def test_inside_on_the_cube():
    v, t, _ = X.cube()
    n = M.pseudo_normals(v, t)
    rng = np.random.default_rng(8)
    p = (rng.random((2000, 3)) * 2.0 - 1.0).astype(F)
    p[:200] *= F(0.45)  # (well inside)
    proj, inside = M.mesh_project(v, t, n, p)
    far = np.linalg.norm(p - proj, axis=1) > 1e-4
    assert far.sum() > 1900
    want = np.abs(p).max(axis=1) <= 0.5
    assert want[far].sum() > 200 and (~want[far]).sum() > 200
    assert np.array_equal(inside[far], want[far])
    # the pseudo-normals of the cube: faces are the axes, an edge's is the sum of two of them, a vertex's is along its diagonal
    assert all(sorted(np.abs(f)) == [0, 0, 1] for f in n["face"])
    kinds = sorted(tuple(sorted(np.abs(e))) for e in n["edge"].values())
    assert kinds == [(0, 0, 2)] * 6 + [(0, 1, 1)] * 12  # (the six face diagonals, the twelve edges of the cube)
    for k in range(8):
        d = n["vertex"][k] / np.linalg.norm(n["vertex"][k])
        assert np.allclose(d, np.sign(v[k]) / np.sqrt(3), atol=1e-6)


def test_heightfield_by_hand():
    """3 rows x 4 columns, scale (3, 2, 4): x = (j / 3 - 0.5) * 3, y = 2 h, z = (i / 2 - 0.5) * 4."""
    h = np.arange(12, dtype=F).reshape(3, 4)
    v, t = M.heightfield_mesh(h, (3.0, 2.0, 4.0))
    third, two_thirds = F(F(1) / F(3)), F(F(2) / F(3))
    xs = [F(-1.5), F(F(third - F(0.5)) * F(3)), F(F(two_thirds - F(0.5)) * F(3)), F(1.5)]
    zs = [F(-2), F(0), F(2)]
    want = np.array([(xs[j], F(2) * h[i, j], zs[i]) for i in range(3) for j in range(4)], F)
    assert np.array_equal(v, want)
    assert len(t) == 12
    assert [tuple(r) for r in t[:4]] == [(0, 4, 5), (0, 5, 1), (1, 5, 6), (1, 6, 2)]
    assert [tuple(r) for r in t[-2:]] == [(6, 10, 11), (6, 11, 7)]
