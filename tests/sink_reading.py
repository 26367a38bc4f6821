"""An independent numpy f64 reading of the regions of DESIGN.md §18 (SalvaHipRegion): the distance of a point to a half-space, a
box, a posed built-in shape, a posed convex oriented mesh and a posed compound, which particles a region selects, and the point
clouds the device tests upload.

A region is a tuple:
    ("halfspace", point, normal)        d = normal . (x - point), with the normal as given (the f32 values the device gets)
    ("aabb", mins, maxs)
    ("shape", shape, t, q)              shape: what salva_amd.coupling.make_shape takes
    ("mesh", (vertices, indices), t, q) CONVEX, closed, counter-clockwise seen from outside: inside = behind every face
    ("compound", parts, t, q)           parts: (shape | ("mesh", vertices, indices, True), t, q) as in tests/compound_reading.py
`signed` is negative inside (minus the depth below the surface); the SOLID distance the library compares with the margin is
max(signed, 0), for a compound the smallest over the parts.  A particle matches when its position is finite and solid <= margin.

The clouds drop every point within 1e-3 r of a decision surface (|signed - margin| < 1e-3 r, for a compound: of any part's) BEFORE
anything is uploaded: coordinates stay within +-2, where the f32 distances of the device err by a few 1e-6 at most against a band of
2.5e-5 at r = 0.025, so the f64 reading and the device agree on every remaining point and no case is left out of the comparison."""
import numpy as np

R = 0.025
BAND = 1.0e-3


def quat_rot(q, v):
    """nalgebra UnitQuaternion * v, f64, q = (i, j, k, w)."""
    q, v = np.asarray(q, np.float64), np.asarray(v, np.float64).reshape(-1, 3)
    u, w = q[:3], q[3]
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def to_local(t, q, pts):
    q = np.asarray(q, np.float64)
    return quat_rot(np.array([-q[0], -q[1], -q[2], q[3]]), np.asarray(pts, np.float64).reshape(-1, 3) - np.asarray(t, np.float64))


def _box_signed(l, he):
    qd = np.abs(l) - np.asarray(he, np.float64)
    return np.linalg.norm(np.maximum(qd, 0.0), axis=1) + np.minimum(qd.max(axis=1), 0.0)


def shape_signed(shape, l):
    x, y, z = l[:, 0], l[:, 1], l[:, 2]
    if shape[0] == "ball":
        return np.sqrt(x * x + y * y + z * z) - float(shape[1])
    if shape[0] == "capsule":
        hh, r = float(shape[1]), float(shape[2])
        ey = y - np.clip(y, -hh, hh)
        return np.sqrt(x * x + ey * ey + z * z) - r
    if shape[0] == "cylinder":
        hh, r = float(shape[1]), float(shape[2])
        dy, dr = np.abs(y) - hh, np.sqrt(x * x + z * z) - r
        return np.hypot(np.maximum(dy, 0.0), np.maximum(dr, 0.0)) + np.minimum(np.maximum(dy, dr), 0.0)
    if shape[0] == "cuboid":
        return _box_signed(l, shape[1])
    raise ValueError(shape)


def _closest_on_triangle(p, a, b, c):
    """Ericson, Real-Time Collision Detection 5.1.5, vectorised over the points p."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = ap @ ab, ap @ ac
    bp = p - b
    d3, d4 = bp @ ab, bp @ ac
    cp = p - c
    d5, d6 = cp @ ab, cp @ ac
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    out = np.empty_like(p)
    done = np.zeros(len(p), bool)

    def take(mask, value):
        m = mask & ~done
        out[m] = value[m] if value.ndim == 2 else value
        done[m] = True

    with np.errstate(divide="ignore", invalid="ignore"):
        take((d1 <= 0) & (d2 <= 0), a)
        take((d3 >= 0) & (d4 <= d3), b)
        take((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + (d1 / (d1 - d3))[:, None] * ab)
        take((d6 >= 0) & (d5 <= d6), c)
        take((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + (d2 / (d2 - d6))[:, None] * ac)
        take((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None] * (c - b))
        den = 1.0 / (va + vb + vc)
        take(np.ones(len(p), bool), a + (vb * den)[:, None] * ab + (vc * den)[:, None] * ac)
    return out


def mesh_signed(vertices, indices, l):
    """A convex oriented mesh: the distance to the closest triangle, negative when the point lies behind every face."""
    v, idx = np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(indices).reshape(-1, 3)
    best = np.full(len(l), np.inf)
    inside = np.ones(len(l), bool)
    for i0, i1, i2 in idx:
        a, b, c = v[i0], v[i1], v[i2]
        best = np.minimum(best, np.linalg.norm(l - _closest_on_triangle(l, a, b, c), axis=1))
        inside &= (l - a) @ np.cross(b - a, c - a) <= 0.0
    return np.where(inside, -best, best)


def _part_signed(shape, l):
    return mesh_signed(shape[1], shape[2], l) if shape[0] == "mesh" else shape_signed(shape, l)


def signed_parts(region, pts):
    """One row per surface the decision can hinge on: [signed distance of every point] per part (one row unless a compound)."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    kind = region[0]
    if kind == "halfspace":
        return ((pts - np.asarray(region[1], np.float64)) @ np.asarray(region[2], np.float64))[None]
    if kind == "aabb":
        lo, hi = np.asarray(region[1], np.float64), np.asarray(region[2], np.float64)
        return _box_signed(pts - 0.5 * (lo + hi), 0.5 * (hi - lo))[None]
    l = to_local(region[2], region[3], pts)
    if kind == "shape":
        return shape_signed(region[1], l)[None]
    if kind == "mesh":
        return mesh_signed(region[1][0], region[1][1], l)[None]
    if kind == "compound":
        return np.stack([_part_signed(shape, to_local(t, q, l)) for shape, t, q in region[1]])
    raise ValueError(kind)


def distance(region, pts):
    """The distance the library compares with the margin: signed for a half-space, solid (0 inside) otherwise."""
    s = signed_parts(region, pts)
    return s[0] if region[0] == "halfspace" else np.maximum(s, 0.0).min(axis=0)


def matches(region, pts, margin):
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    finite = np.isfinite(pts).all(axis=1)
    with np.errstate(invalid="ignore"):
        return finite & (distance(region, np.where(finite[:, None], pts, 0.0)) <= margin)


def selected(region, pts, margin, invert=False):
    """The particles a region deletes."""
    m = matches(region, pts, margin)
    return ~m if invert else m


def in_band(region, pts, margin, r=R):
    """Within 1e-3 r of a surface the decision hinges on."""
    return (np.abs(signed_parts(region, pts) - margin) < BAND * r).any(axis=0)


def bounds(region):
    """A box around the region, inside +-2."""
    kind = region[0]
    if kind == "halfspace":
        c = np.asarray(region[1], np.float64)
        return c - 0.6, c + 0.6
    if kind == "aabb":
        return np.asarray(region[1], np.float64) - 0.25, np.asarray(region[2], np.float64) + 0.25
    c = np.asarray(region[2], np.float64)
    return c - 0.7, c + 0.7


def cloud(region, n, margins, seed, r=R):
    """n f32 points around the region, none of them in the band of any of `margins`."""
    rng = np.random.default_rng(seed)
    lo, hi = bounds(region)
    assert (lo > -2.0).all() and (hi < 2.0).all()
    out = np.zeros((0, 3), np.float32)
    while len(out) < n:
        p = (lo + rng.random((2 * n, 3)) * (hi - lo)).astype(np.float32)
        ok = np.ones(len(p), bool)
        for m in margins:
            ok &= ~in_band(region, p, m, r)
        out = np.concatenate([out, p[ok]])
    return np.ascontiguousarray(out[:n])


# ---- the regions the tests share -----------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(np.float32)


Q = _unit([0.2, -0.3, 0.1, 0.9])
OCTA_V = np.array([[0.5, 0, 0], [-0.5, 0, 0], [0, 0.4, 0], [0, -0.4, 0], [0, 0, 0.45], [0, 0, -0.45]], np.float32)
OCTA_I = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.uint32)
T = np.array([0.1, -0.05, 0.15], np.float32)
COMPOUND_PARTS = [
    (("ball", 0.3), np.array([-0.3, 0.0, 0.0], np.float32), np.array([0, 0, 0, 1], np.float32)),
    (("cuboid", (0.25, 0.15, 0.2)), np.array([0.25, 0.1, 0.0], np.float32), _unit([0.1, 0.2, -0.1, 0.95])),
    (("mesh", (OCTA_V * np.float32(0.6)).astype(np.float32), OCTA_I, True), np.array([0.0, -0.2, 0.25], np.float32), _unit([-0.2, 0.1, 0.3, 0.9])),
]
REGIONS = {
    "halfspace": ("halfspace", np.array([0.1, -0.2, 0.05], np.float32), _unit([0.3, 1.0, -0.2])),
    "aabb": ("aabb", np.array([-0.5, -0.3, -0.4], np.float32), np.array([0.4, 0.5, 0.3], np.float32)),
    "ball": ("shape", ("ball", 0.5), T, Q),
    "cuboid": ("shape", ("cuboid", (0.4, 0.3, 0.5)), T, Q),
    "capsule": ("shape", ("capsule", 0.3, 0.25), T, Q),
    "cylinder": ("shape", ("cylinder", 0.35, 0.3), T, Q),
    "mesh": ("mesh", (OCTA_V, OCTA_I), T, Q),
    "compound": ("compound", COMPOUND_PARTS, T, Q),
}


def to_api(region, margin=0.0, invert=False):
    """The same region as a salva_amd.regions object."""
    from salva_amd import regions, sampling

    kind = region[0]
    if kind == "halfspace":
        return regions.HalfSpace(region[1], region[2], margin, invert)
    if kind == "aabb":
        return regions.Aabb(region[1], region[2], margin, invert)
    if kind == "shape":
        return regions.Shape(region[1], region[2], region[3], margin, invert)
    if kind == "mesh":
        return regions.Mesh(sampling.Mesh(region[1][0], region[1][1], oriented=True), region[2], region[3], margin, invert)
    parts = [(sampling.Mesh(s[1], s[2], oriented=s[3]) if s[0] == "mesh" else s, t, q) for s, t, q in region[1]]
    return regions.Compound(sampling.Compound(parts), region[2], region[3], margin, invert)
