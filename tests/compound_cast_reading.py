"""An independent numpy f32 reading of the general-direction ray casts of DESIGN.md §17 "Ray sampling" (salva_amd/csrc/raycast.h)
and of the ray sampler on a compound (sample.hip k_compound_mark): operation by operation, a brute force over ALL parts and ALL
triangles — no boxes, no hierarchy, no pruning.  What the device is compared with bit for bit.  The lattice and the quantisation
are tests/sampling_reading.py's, poses and parts tests/compound_reading.py's, the edge function tests/mesh_reading.py's.

One rule for every kind: the cast of o + t d at a part is the smallest t >= 0 at which the ray crosses the part's boundary, +inf for
a miss; the compound's is the smallest over its parts.  A convex part is an interval [t0, t1] (empty: [+inf, -inf])."""
import numpy as np

import compound_reading as CR
import compound_scenes as CS
import mesh_reading as M
import sampling_reading as R
from test_host_shape_gpu import quat_rot

F = np.float32
INF = F(np.inf)
MAX_HITS = 64


def _dot(ax, ay, az, bx, by, bz):
    return ((ax * bx) + (ay * by)) + (az * bz)


def crossing(t0, t1):
    with np.errstate(invalid="ignore"):
        return np.where(t0 >= 0, t0, np.where(t1 >= 0, t1, INF)).astype(F)


def ball_iv(o, d, r):
    """About the point of closest approach: tm = -(o.d) / (d.d), p = o + tm d, disc = r r - p.p, half = sqrt(disc / (d.d))."""
    r = F(r)
    ox, oy, oz, dx, dy, dz = o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]
    a, b = _dot(dx, dy, dz, dx, dy, dz), _dot(ox, oy, oz, dx, dy, dz)
    tm = (-b) / a
    px, py, pz = ox + (tm * dx), oy + (tm * dy), oz + (tm * dz)
    disc = (r * r) - _dot(px, py, pz, px, py, pz)
    ok = disc > 0
    half = np.sqrt(disc / a)
    return np.where(ok, tm - half, INF).astype(F), np.where(ok, tm + half, -INF).astype(F)


def _slab(o, d, h, t0, t1):
    """|x| <= h intersected into [t0, t1] -> (the ray does not run beside the slab, t0, t1)."""
    h = F(h)
    flat = d == 0
    u, v = ((-h) - o) / d, (h - o) / d
    n0, n1 = np.maximum(t0, np.minimum(u, v)), np.minimum(t1, np.maximum(u, v))
    return np.where(flat, np.abs(o) <= h, True), np.where(flat, t0, n0).astype(F), np.where(flat, t1, n1).astype(F)


def cuboid_iv(o, d, he):
    a, b = np.full(len(o), -INF, F), np.full(len(o), INF, F)
    on = np.ones(len(o), bool)
    for k in range(3):
        ok, a, b = _slab(o[:, k], d[:, k], he[k], a, b)
        on &= ok
    hit = on & (a <= b)
    return np.where(hit, a, INF).astype(F), np.where(hit, b, -INF).astype(F)


def cylinder_iv(o, d, hh, r):
    """The side's quadratic in the (x, z) plane intersected with the slab |y| <= hh."""
    r = F(r)
    ox, oy, oz, dx, dy, dz = o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]
    a = (dx * dx) + (dz * dz)
    slanted = a > 0
    b = (ox * dx) + (oz * dz)
    tm = (-b) / a
    px, pz = ox + (tm * dx), oz + (tm * dz)
    disc = (r * r) - ((px * px) + (pz * pz))
    half = np.sqrt(disc / a)
    side = np.where(slanted, disc > 0, ((r * r) - ((ox * ox) + (oz * oz))) > 0)
    s0, s1 = np.where(slanted, tm - half, -INF).astype(F), np.where(slanted, tm + half, INF).astype(F)
    on, s0, s1 = _slab(oy, dy, hh, s0, s1)
    hit = side & on & (s0 <= s1)
    return np.where(hit, s0, INF).astype(F), np.where(hit, s1, -INF).astype(F)


def capsule_iv(o, d, hh, r):
    """The hull of three intervals: the cylinder's and the balls' about (0, +-hh, 0)."""
    hh = F(hh)
    t0, t1 = cylinder_iv(o, d, hh, r)
    up, down = o.copy(), o.copy()
    up[:, 1], down[:, 1] = o[:, 1] - hh, o[:, 1] + hh
    a0, a1 = ball_iv(up, d, r)
    b0, b1 = ball_iv(down, d, r)
    return np.minimum(t0, np.minimum(a0, b0)), np.maximum(t1, np.maximum(a1, b1))


def shape_cast(shape, o, d):
    """A ball, a cuboid, a capsule or a cylinder in its own frame."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if shape[0] == "ball":
            t0, t1 = ball_iv(o, d, shape[1])
        elif shape[0] == "cuboid":
            t0, t1 = cuboid_iv(o, d, [F(x) for x in shape[1]])
        elif shape[0] == "capsule":
            t0, t1 = capsule_iv(o, d, shape[1], shape[2])
        else:
            t0, t1 = cylinder_iv(o, d, shape[1], shape[2])
    return crossing(t0, t1)


def _pick(k, x, y, z):
    return np.where(k == 0, x, np.where(k == 1, y, z))


def mesh_cast(vertices, indices, o, d, best=None, counts=None):
    """The smallest t in [0, best) over all triangles, `best` where there is none.  Every triangle in the frame sheared along the
    ray's dominant axis; the edge functions at (0, 0) with the endpoints in vertex-index order; t clamped to the vertices' Z."""
    v, tri = np.asarray(vertices, F), np.asarray(indices, np.int64)
    n = len(o)
    best = np.full(n, INF, F) if best is None else best
    ad = np.abs(d)
    kz = np.where((ad[:, 0] >= ad[:, 1]) & (ad[:, 0] >= ad[:, 2]), 0, np.where(ad[:, 1] >= ad[:, 2], 1, 2))
    dk = _pick(kz, d[:, 0], d[:, 1], d[:, 2])
    sx, sy, sz = _pick(kz, d[:, 1], d[:, 2], d[:, 0]) / dk, _pick(kz, d[:, 2], d[:, 0], d[:, 1]) / dk, F(1.0) / dk
    px, py, pz = _pick(kz, o[:, 1], o[:, 2], o[:, 0]), _pick(kz, o[:, 2], o[:, 0], o[:, 1]), _pick(kz, o[:, 0], o[:, 1], o[:, 2])
    A = v[:, kz].T - pz[:, None]                                   # (n, nv)
    X = (v[:, (kz + 1) % 3].T - px[:, None]) - (sx[:, None] * A)
    Y = (v[:, (kz + 2) % 3].T - py[:, None]) - (sy[:, None] * A)
    Z = sz[:, None] * A
    i0, i1, i2 = tri[:, 0], tri[:, 1], tri[:, 2]
    X0, X1, X2, Y0, Y1, Y2, Z0, Z1, Z2 = X[:, i0], X[:, i1], X[:, i2], Y[:, i0], Y[:, i1], Y[:, i2], Z[:, i0], Z[:, i1], Z[:, i2]
    zero = F(0.0)
    e0, e1, e2 = M._edge(i1, i2, X1, Y1, X2, Y2, zero, zero), M._edge(i2, i0, X2, Y2, X0, Y0, zero, zero), M._edge(i0, i1, X0, Y0, X1, Y1, zero, zero)
    total = (e0 + e1) + e2
    boxed = ((np.minimum(np.minimum(X0, X1), X2) <= 0) & (np.maximum(np.maximum(X0, X1), X2) >= 0)
             & (np.minimum(np.minimum(Y0, Y1), Y2) <= 0) & (np.maximum(np.maximum(Y0, Y1), Y2) >= 0))
    hit = (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))) & (total != 0) & boxed
    with np.errstate(divide="ignore", invalid="ignore"):
        h = (((e0 * Z0) + (e1 * Z1)) + (e2 * Z2)) / total
        t = np.minimum(np.maximum(h, np.minimum(np.minimum(Z0, Z1), Z2)), np.maximum(np.maximum(Z0, Z1), Z2))
        ok = hit & (t >= 0) & (t < best[:, None])
    if counts is not None:
        counts.append(ok.sum(axis=1))
    return np.minimum(best, np.where(ok, t, INF).min(axis=1)).astype(F)


def part_frame(part, o, d):
    """The ray in the part's frame: quat_rot with the conjugate on o - t_k and on d."""
    _, t, q = part
    q = np.asarray(q, F)
    conj = (-q[0], -q[1], -q[2], q[3])
    return quat_rot(conj, (o - np.asarray(t, F)).astype(F)), quat_rot(conj, d)


def part_cast(part, o, d):
    """One part alone, the ray given in the compound's frame."""
    l, e = part_frame(part, o, d)
    shape = part[0]
    return mesh_cast(shape[1], shape[2], l, e) if shape[0] == "mesh" else shape_cast(shape, l, e)


def compound_cast(parts, o, d, winners=None):
    """Every part in index order, the smallest t; +inf: a miss."""
    o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
    best, who = np.full(len(o), INF, F), np.full(len(o), -1)
    for k, part in enumerate(parts):
        t = part_cast(part, o, d)
        win = t < best
        best, who = np.where(win, t, best).astype(F), np.where(win, k, who)
    if winners is not None:
        winners.append(who)
    return best


def axis_dirs(n, axis):
    d = np.zeros((n, 3), F)
    d[:, axis] = 1
    return d


def cast_axis(parts, origins, axis):
    """The callback a HostRayShape wants: toi of the rays from `origins` along +axis, -1 for a miss."""
    origins = np.asarray(origins, F).reshape(-1, 3)
    t = compound_cast(parts, origins, axis_dirs(len(origins), axis))
    return np.where(t < INF, t, F(-1.0)).astype(F)


def sample_with_cast(mins, maxs, particle_rad, mode, cast, hits_per_ray=None, step=None):
    """The loop of World::sample_host_shape / k_sample_mesh_mark around `cast(origins, axis) -> toi (-1: a miss)`: impact = origin +
    toi, the next origin = origin + (toi + s / 10), entry and exit alternating.  -> (indices, positions, N)."""
    s, origin, coords = R.lattice(mins, maxs, particle_rad)
    N = [len(c) for c in coords]
    step = F(s / F(10.0)) if step is None else F(step)
    out = set()
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        cj, ck = np.meshgrid(np.asarray(coords[j], F), np.asarray(coords[k], F), indexing="ij")
        cj, ck = cj.ravel(), ck.ravel()
        org = np.empty((len(cj), 3), F)
        org[:, i], org[:, j], org[:, k] = origin[i], cj, ck
        qj = [R.as_u32(R.roundf(F(F(c - origin[j]) / s))) for c in cj]
        qk = [R.as_u32(R.roundf(F(F(c - origin[k]) / s))) for c in ck]
        live = np.arange(len(cj))
        entry, prev, count = np.ones(len(cj), bool), {}, np.zeros(len(cj), np.int64)
        while len(live):
            toi = cast(org[live], i)
            keep = []
            for r, t in zip(live, toi):
                if not t >= 0:
                    continue
                count[r] += 1
                assert count[r] <= MAX_HITS, "a ray with more than 64 accepted hits"
                oi = org[r, i]
                impact = F(oi + t)
                q = [0, 0, 0]
                q[j], q[k] = qj[r], qk[r]

                def put(qi):
                    q[i] = qi
                    if q[0] < N[0] and q[1] < N[1] and q[2] < N[2]:
                        out.add(tuple(q))

                f = F(F(impact - origin[i]) / s)
                if mode == R.SURFACE:
                    put(R.as_u32(np.ceil(f) if entry[r] else np.floor(f)))
                    entry[r] = not entry[r]
                elif r in prev:
                    q0 = R.as_u32(R.roundf(F(F(prev.pop(r) - origin[i]) / s)))
                    for qi in range(q0, min(R.as_u32(R.roundf(f)), N[i] - 1) + 1):
                        put(qi)
                else:
                    prev[r] = impact
                org[r, i] = F(oi + F(t + step))
                keep.append(r)
            live = np.asarray(keep, np.int64)
        if hits_per_ray is not None:
            hits_per_ray.extend(count.tolist())
    q, pos = R._unquantise(out, s, origin)
    return q, pos, N


def sample(parts, particle_rad, mode, hits_per_ray=None):
    """The compound's lattice is that of its local box, the unloosened merge of the parts' boxes."""
    mins, maxs = CR.local_aabb(parts)
    return sample_with_cast(mins, maxs, particle_rad, mode, lambda origins, axis: cast_axis(parts, origins, axis), hits_per_ray)


# ------------------------------------------------------------------------------------------------ scenes
def ring_compound(count=64):
    """64 small cuboids, each rotated differently, on a circle of radius 0.5 in the plane through the origin with normal (1, 1, 1).
    They do not touch — centres 0.049 apart, 0.0242 from a centre to a corner — and no lattice ray crosses the ring twice: an axis
    meets the ring's plane once, at 55 degrees to its normal.  So when a chord shorter than s / 10 loses its exit (§13's thin-chord
    rule) and the ray's next hit is paired with its entry, as the reference's loop pairs them, the stretch filled in volume mode
    spans a gap between neighbours, about one lattice spacing wide, and not the inside of the ring."""
    u, v, n = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0), np.array([1.0, 1.0, -2.0]) / np.sqrt(6.0), np.ones(3) / np.sqrt(3.0)
    parts = []
    for k in range(count):
        ang = 2.0 * np.pi * k / count
        centre = 0.5 * (np.cos(ang) * u + np.sin(ang) * v) + 0.01 * np.sin(3 * ang) * n
        parts.append((("cuboid", (0.014, 0.017, 0.01)), F(centre), CS.quat((0.9 * np.sin(ang), -ang, 0.4 + 0.1 * k))))
    return parts


SCENES = {"body_compound": CS.body_compound, "slab_compound": CS.slab_compound, "far_apart": CS.far_apart, "ring": ring_compound}
RAD = 0.0125
