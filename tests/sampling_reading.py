"""An independent numpy f32 reading of the ray sampler's specification (src/sampling/ray_sampling.rs of the
reference with parry's casts replaced by closed forms): four analytic shapes, both modes, the thin-chord rule, and interval lists
for shapes the library casts at through the host.  Scalar loops on purpose: this file is what the device kernels are compared with
bit for bit, so it shares nothing with them and nothing with salva_amd/scenes.py.

Every operation is a correctly rounded f32 operation; `round` is half away from zero (Rust's f32::round, C's roundf), not numpy's.
"""
import math

import numpy as np

F = np.float32
SURFACE, VOLUME = 0, 1


def roundf(x) -> float:
    """f32::round: half away from zero."""
    x = float(x)
    return math.floor(x + 0.5) if x >= 0.0 else -math.floor(-x + 0.5)


def as_u32(x) -> int:
    """Rust's `as u32` of a float: saturating, NaN -> 0."""
    x = float(x)
    if not x > 0.0:
        return 0
    return min(int(x), 0xFFFFFFFF)


def half_extents(shape):
    kind = shape[0]
    if kind == "ball":
        return [F(shape[1])] * 3
    if kind == "cuboid":
        return [F(v) for v in shape[1]]
    hh, R = F(shape[1]), F(shape[2])
    if kind == "capsule":
        return [R, F(hh + R), R]
    if kind == "cylinder":
        return [R, hh, R]
    raise ValueError(kind)


def lattice(mins, maxs, particle_rad):
    """-> (s, origin[3], coords[3]): the lattice lines of each axis, accumulated by repeated f32 addition."""
    s = F(F(particle_rad) * F(2.0))
    origin, coords = [], []
    for a in range(3):
        lo, hi = F(F(mins[a]) - s), F(F(maxs[a]) + s)
        o = F(lo + F(s / F(2.0)))
        line, c = [], o
        while c < hi:
            line.append(c)
            c = F(c + s)
        origin.append(o)
        coords.append(line)
    return s, origin, coords


def cast(shape, i, cj, ck):
    """The ray along +axis i through (c_j, c_k), j = i + 1, k = i + 2 mod 3 -> (a, b) or None."""
    kind = shape[0]
    if kind == "ball":
        R = F(shape[1])
        d2 = F(F(R * R) - F(F(cj * cj) + F(ck * ck)))
        if not d2 > 0:
            return None
        h = F(np.sqrt(d2))
        return F(-h), h
    if kind == "cuboid":
        he = [F(v) for v in shape[1]]
        j, k = (i + 1) % 3, (i + 2) % 3
        if not (abs(cj) <= he[j] and abs(ck) <= he[k]):
            return None
        return F(-he[i]), he[i]
    hh, R = F(shape[1]), F(shape[2])
    c = [None, None, None]
    c[(i + 1) % 3], c[(i + 2) % 3] = cj, ck
    if i == 1:
        d2 = F(F(R * R) - F(F(c[0] * c[0]) + F(c[2] * c[2])))
        if kind == "cylinder":
            if not d2 >= 0:
                return None
            return F(-hh), hh
        if not d2 > 0:
            return None
        b = F(hh + F(np.sqrt(d2)))
        return F(-b), b
    cy, co = c[1], c[2] if i == 0 else c[0]
    if kind == "cylinder":
        d2 = F(F(R * R) - F(co * co))
        if not (abs(cy) <= hh and d2 > 0):
            return None
    else:
        dy = max(F(abs(cy) - hh), F(0.0))
        d2 = F(F(F(R * R) - F(dy * dy)) - F(co * co))
        if not d2 > 0:
            return None
    h = F(np.sqrt(d2))
    return F(-h), h


def _quantise(index_set, N, s, origin, i, cj, ck, intervals, mode, record=None):
    """One ray's impacts -> lattice indices.  `intervals`: [(a, b or None), ...] in ray order; b = None: no exit was found (the
    second cast started beyond the shape)."""
    j, k = (i + 1) % 3, (i + 2) % 3
    q = [0, 0, 0]
    q[j] = as_u32(roundf(F(F(cj - origin[j]) / s)))
    q[k] = as_u32(roundf(F(F(ck - origin[k]) / s)))

    def put(qi):
        q[i] = qi
        if q[0] < N[0] and q[1] < N[1] and q[2] < N[2]:
            index_set.add(tuple(q))
            if record is not None:
                record.append(tuple(q))

    for a, b in intervals:
        fa = F(F(a - origin[i]) / s)
        if mode == SURFACE:
            put(as_u32(math.ceil(fa)))
            if b is not None:
                put(as_u32(math.floor(F(F(b - origin[i]) / s))))
        elif b is not None:
            for qi in range(as_u32(roundf(fa)), min(as_u32(roundf(F(F(b - origin[i]) / s))), N[i] - 1) + 1):
                put(qi)


def _unquantise(index_set, s, origin):
    """-> (indices (n, 3) int64, positions (n, 3) f32) in lexicographic index order."""
    q = np.asarray(sorted(index_set), dtype=np.int64).reshape(-1, 3)
    pos = np.empty((len(q), 3), F)
    for a in range(3):
        pos[:, a] = origin[a] + q[:, a].astype(F) * s
    return q, pos


def thin(a, b, s) -> bool:
    """The reference casts again from impact + s / 10: a chord shorter than that has no exit impact."""
    return bool(F(b - a) < F(s / F(10.0)))


def sample(shape, particle_rad, mode, per_axis=None):
    """shape: ("ball", R) | ("cuboid", (hx, hy, hz)) | ("capsule", hh, R) | ("cylinder", hh, R).
    -> (indices, positions, N).  per_axis (a dict) receives {axis: [index tuples that axis's rays produced]}."""
    ext = half_extents(shape)
    s, origin, coords = lattice([F(-e) for e in ext], ext, particle_rad)
    N = [len(c) for c in coords]
    out = set()
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        rec = [] if per_axis is not None else None
        for cj in coords[j]:
            for ck in coords[k]:
                hit = cast(shape, i, cj, ck)
                if hit is None:
                    continue
                a, b = hit
                _quantise(out, N, s, origin, i, cj, ck, [(a, None if thin(a, b, s) else b)], mode, rec)
        if per_axis is not None:
            per_axis[i] = rec
    q, pos = _unquantise(out, s, origin)
    return q, pos, N


def sample_intervals(mins, maxs, particle_rad, mode, intervals_of):
    """A shape given by its aabb and `intervals_of(axis, c_j, c_k) -> [(a, b), ...]` (ascending, disjoint): concave shapes."""
    s, origin, coords = lattice(mins, maxs, particle_rad)
    N = [len(c) for c in coords]
    out = set()
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        for cj in coords[j]:
            for ck in coords[k]:
                iv = [(F(a), None if thin(F(a), F(b), s) else F(b)) for a, b in intervals_of(i, cj, ck)]
                _quantise(out, N, s, origin, i, cj, ck, iv, mode)
    q, pos = _unquantise(out, s, origin)
    return q, pos, N


def ray_chords(shape, particle_rad):
    """[(axis, c_j, c_k, a, b)] of every hitting ray."""
    ext = half_extents(shape)
    s, origin, coords = lattice([F(-e) for e in ext], ext, particle_rad)
    rays = []
    for i in range(3):
        for cj in coords[(i + 1) % 3]:
            for ck in coords[(i + 2) % 3]:
                hit = cast(shape, i, cj, ck)
                if hit is not None:
                    rays.append((i, cj, ck, hit[0], hit[1]))
    return rays, s, origin, coords


def find_thin_chord_ball(particle_rad=0.0125, start=0.1, tries=4000):
    """A ball radius with at least one ray of chord 0 < b - a < s / 10: R slightly above the distance of some lattice line from the
    centre.  Found by search over R in steps of 1e-5; deterministic."""
    s = F(F(particle_rad) * F(2.0))
    for t in range(tries):
        R = float(F(start + 1e-5 * t))
        rays, s, _, _ = ray_chords(("ball", R), particle_rad)
        if any(0 < F(b - a) < F(s / F(10.0)) for _, _, _, a, b in rays):
            return R
    raise AssertionError("no thin-chord radius found")


def two_balls_intervals(R=0.1, dx=0.15):
    """Two balls of radius R with centres at x = -dx and x = +dx (0.3 apart for dx = 0.15): the intervals of a ray, in f32.
    Along x a ray through both has two disjoint intervals; along y / z a ray meets one ball at most (they do not overlap)."""
    R, dx = F(R), F(dx)

    def intervals_of(i, cj, ck):
        out = []
        for cx in (F(-dx), dx):
            c = [None, None, None]
            c[(i + 1) % 3], c[(i + 2) % 3] = cj, ck
            if i == 0:
                d2 = F(F(R * R) - F(F(c[1] * c[1]) + F(c[2] * c[2])))
                centre = cx
            else:
                ex = F(c[0] - cx)
                other = c[2] if i == 1 else c[1]
                d2 = F(F(R * R) - F(F(ex * ex) + F(other * other)))
                centre = F(0.0)
            if d2 > 0:
                h = F(np.sqrt(d2))
                out.append((F(centre - h), F(centre + h)))
        return out

    mins = [F(-dx - R), F(-R), F(-R)]
    maxs = [F(dx + R), R, R]
    return mins, maxs, intervals_of
