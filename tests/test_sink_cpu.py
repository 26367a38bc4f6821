"""tests/sink_reading.py against closed cases (no GPU): the five distances of DESIGN.md §18 at points whose distance is known by
hand, and the clouds the device tests upload - every kind keeps matches and non-matches, plain and inverted, at both margins."""
import numpy as np
import pytest

import sink_reading as S

I4 = np.array([0, 0, 0, 1], np.float32)
Z3 = np.zeros(3, np.float32)


def d(region, p):
    return float(S.distance(region, np.array([p], np.float64))[0])


def test_halfspace_is_the_signed_plane_distance():
    hs = ("halfspace", [0.0, 1.0, 0.0], [0.0, 1.0, 0.0])
    assert d(hs, [3.0, 1.5, -2.0]) == pytest.approx(0.5) and d(hs, [0.0, -1.0, 0.0]) == pytest.approx(-2.0)
    assert S.matches(hs, [[0, 0.9, 0], [0, 1.1, 0], [0, 1.1, np.nan]], 0.0).tolist() == [True, False, False]
    assert S.selected(hs, [[0, 0.9, 0], [0, 1.1, 0], [np.inf, 0, 0]], 0.0, invert=True).tolist() == [False, True, True]


def test_box_and_cuboid_at_face_edge_and_corner():
    box = ("aabb", [-1.0, -1.0, -1.0], [1.0, 2.0, 1.0])
    assert d(box, [0.0, 0.0, 0.0]) == 0.0 and d(box, [1.5, 0.0, 0.0]) == pytest.approx(0.5)
    assert d(box, [1.0 + 3.0, 2.0 + 4.0, 1.0 + 12.0]) == pytest.approx(13.0)  # a corner
    cub = ("shape", ("cuboid", (0.5, 0.25, 1.0)), [1.0, 0.0, 0.0], I4)
    assert d(cub, [1.0, 0.0, 0.0]) == 0.0 and d(cub, [1.8, 0.65, 0.0]) == pytest.approx(0.5)  # an edge: (0.3, 0.4)
    assert float(S.signed_parts(cub, [[1.0, 0.0, 0.0]])[0, 0]) == pytest.approx(-0.25)


def test_round_shapes_on_their_axes():
    assert d(("shape", ("ball", 0.5), Z3, I4), [2.0, 0.0, 0.0]) == pytest.approx(1.5)
    cap = ("shape", ("capsule", 0.3, 0.25), Z3, I4)
    assert d(cap, [0.0, 1.0, 0.0]) == pytest.approx(1.0 - 0.3 - 0.25) and d(cap, [1.0, 0.1, 0.0]) == pytest.approx(0.75)
    cyl = ("shape", ("cylinder", 0.35, 0.3), Z3, I4)
    assert d(cyl, [0.0, 1.0, 0.0]) == pytest.approx(0.65) and d(cyl, [0.7, 0.0, 0.0]) == pytest.approx(0.4)
    assert d(cyl, [0.3 + 0.3, 0.35 + 0.4, 0.0]) == pytest.approx(0.5) and d(cyl, [0.1, 0.1, 0.1]) == 0.0  # the rim; inside
    # a quarter turn about z lays the capsule's axis along x
    s = np.float32(np.sqrt(0.5))
    assert d(("shape", ("capsule", 0.3, 0.25), Z3, np.array([0, 0, s, s], np.float32)), [1.0, 0.0, 0.0]) == pytest.approx(0.45, abs=1e-6)


def test_mesh_is_convex_oriented_and_reads_like_its_faces():
    v, idx = S.OCTA_V.astype(np.float64), S.OCTA_I
    for i0, i1, i2 in idx:  # counter-clockwise seen from outside: the normal points away from the centre
        assert np.cross(v[i1] - v[i0], v[i2] - v[i0]) @ (v[i0] + v[i1] + v[i2]) > 0
    m = ("mesh", (S.OCTA_V, S.OCTA_I), Z3, I4)
    assert d(m, [0.0, 0.0, 0.0]) == 0.0 and d(m, [1.5, 0.0, 0.0]) == pytest.approx(1.0)  # the vertex on the axis
    n = np.cross(v[2] - v[0], v[4] - v[0])
    n /= np.linalg.norm(n)
    c = (v[0] + v[2] + v[4]) / 3.0
    assert d(m, c + 0.2 * n) == pytest.approx(0.2) and float(S.signed_parts(m, [c - 0.01 * n])[0, 0]) == pytest.approx(-0.01)


def test_compound_is_the_smallest_of_its_parts():
    parts = [(("ball", 0.3), [-1.0, 0.0, 0.0], I4), (("cuboid", (0.2, 0.2, 0.2)), [1.0, 0.0, 0.0], I4)]
    c = ("compound", parts, Z3, I4)
    assert d(c, [-1.1, 0.1, 0.0]) == 0.0 and d(c, [1.0, 0.1, 0.1]) == 0.0  # inside a part
    assert d(c, [0.0, 0.0, 0.0]) == pytest.approx(0.7) and d(c, [0.3, 0.0, 0.0]) == pytest.approx(0.5)
    moved = ("compound", parts, [0.0, 2.0, 0.0], I4)
    assert d(moved, [0.0, 2.0, 0.0]) == pytest.approx(0.7)


@pytest.mark.parametrize("name", sorted(S.REGIONS))
def test_clouds_keep_both_sides_and_stay_out_of_the_band(name):
    region = S.REGIONS[name]
    margins = (0.0, S.R)
    pts = S.cloud(region, 2603, margins, seed=7)
    assert pts.dtype == np.float32 and pts.shape == (2603, 3) and np.abs(pts).max() < 2.0
    for m in margins:
        assert not S.in_band(region, pts, m).any()
        for invert in (False, True):
            sel = S.selected(region, pts, m, invert)
            assert 100 < sel.sum() < len(pts) - 100, (name, m, invert, int(sel.sum()))
    # the two margins select different sets: the shell between them is populated
    assert (S.matches(region, pts, S.R) & ~S.matches(region, pts, 0.0)).sum() > 5
