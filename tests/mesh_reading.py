"""An independent numpy reading of the triangle-mesh geometry of DESIGN.md §14: the cast of an axis-parallel ray, the closest
point with its feature, parry's height field as triangles and the pseudo-normals.  f32 operation by operation (numpy rounds every
elementwise operation on float32 arrays once and never fuses), brute force over all triangles, no hierarchy: what the device
kernels of salva_amd/csrc/mesh.h are compared with bit for bit.  Shares nothing with them."""
import numpy as np

import sampling_reading as R

F = np.float32
INF = F(np.inf)


# ------------------------------------------------------------------------------------------------ height field, pseudo-normals
def heightfield_mesh(heights, scale):
    """-> (vertices (nrows * ncols, 3) f32, indices (2 (nrows - 1) (ncols - 1), 3) uint32)."""
    heights = np.asarray(heights, F)
    nrows, ncols = heights.shape
    sx, sy, sz = (F(v) for v in scale)
    v = np.empty((nrows * ncols, 3), F)
    tris = []
    for i in range(nrows):
        for j in range(ncols):
            v[i * ncols + j] = (F(F(F(j) / F(ncols - 1)) - F(0.5)) * sx, heights[i, j] * sy, F(F(F(i) / F(nrows - 1)) - F(0.5)) * sz)
    for i in range(nrows - 1):
        for j in range(ncols - 1):
            p00, p01, p10, p11 = i * ncols + j, i * ncols + j + 1, (i + 1) * ncols + j, (i + 1) * ncols + j + 1
            tris += [(p00, p10, p11), (p00, p11, p01)]
    return v, np.asarray(tris, np.uint32)


def pseudo_normals(vertices, indices):
    """f64 -> {"face": (nt, 3) f32, "vertex": (nv, 3) f32, "edge": {(lo, hi): (3,) f32}}: the unit face normal; per edge the sum of
    the unit normals of the faces at it; per vertex the sum of the unit normals of the faces around it weighted by their angle there."""
    v = np.asarray(vertices, np.float64)
    face = np.zeros((len(indices), 3))
    vert = np.zeros((len(v), 3))
    edge = {}
    for t, tri in enumerate(np.asarray(indices, np.int64)):
        p = v[tri]
        n = np.cross(p[1] - p[0], p[2] - p[0])
        ln = np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
        n = n / ln if ln > 0 else np.zeros(3)
        face[t] = n
        for c in range(3):
            e1, e2 = p[(c + 1) % 3] - p[c], p[(c + 2) % 3] - p[c]
            cr = np.cross(e1, e2)
            angle = np.arctan2(np.sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]), e1[0] * e2[0] + e1[1] * e2[1] + e1[2] * e2[2])
            vert[tri[c]] += angle * n
            key = (int(min(tri[c], tri[(c + 1) % 3])), int(max(tri[c], tri[(c + 1) % 3])))
            edge[key] = edge.get(key, np.zeros(3)) + n
    return {"face": face.astype(F), "vertex": vert.astype(F), "edge": {k: e.astype(F) for k, e in edge.items()}}


# ------------------------------------------------------------------------------------------------ the cast
def _edge(ia, ib, aj, ak, bj, bk, cj, ck):
    """The edge function of c against a -> b, the endpoints taken in the order of their vertex indices; (T,) against (n, 1)."""
    swap = ia > ib
    pj, pk, qj, qk = np.where(swap, bj, aj), np.where(swap, bk, ak), np.where(swap, aj, bj), np.where(swap, ak, bk)
    e = ((qj - pj) * (ck - pk)) - ((qk - pk) * (cj - pj))
    return np.where(swap, -e, e)


def mesh_hits(vertices, indices, axis, cj, ck):
    """-> (n, T) f32: the hit coordinate of every ray (c_j, c_k) with every triangle, NaN where the ray misses."""
    v, tri = np.asarray(vertices, F), np.asarray(indices, np.int64)
    j, k = (axis + 1) % 3, (axis + 2) % 3
    cj, ck = np.asarray(cj, F).reshape(-1, 1), np.asarray(ck, F).reshape(-1, 1)
    i0, i1, i2 = tri[:, 0], tri[:, 1], tri[:, 2]
    p0, p1, p2 = v[i0], v[i1], v[i2]
    e0 = _edge(i1, i2, p1[:, j], p1[:, k], p2[:, j], p2[:, k], cj, ck)
    e1 = _edge(i2, i0, p2[:, j], p2[:, k], p0[:, j], p0[:, k], cj, ck)
    e2 = _edge(i0, i1, p0[:, j], p0[:, k], p1[:, j], p1[:, k], cj, ck)
    total = (e0 + e1) + e2
    hit = (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))) & (total != 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = (((e0 * p0[:, axis]) + (e1 * p1[:, axis])) + (e2 * p2[:, axis])) / total
    return np.where(hit, h, F(np.nan)).astype(F)


def mesh_cast(vertices, indices, origins, axis):
    """`cast_local_ray` of the rays from `origins` along +axis: toi = (the smallest hit coordinate >= the origin) - the origin, -1 for a miss."""
    origins = np.asarray(origins, F).reshape(-1, 3)
    j, k = (axis + 1) % 3, (axis + 2) % 3
    h = mesh_hits(vertices, indices, axis, origins[:, j], origins[:, k])
    o = origins[:, axis]
    with np.errstate(invalid="ignore"):
        h = np.where(h >= o[:, None], h, INF)
    best = h.min(axis=1) if h.shape[1] else np.full(len(o), INF)
    with np.errstate(invalid="ignore"):
        return np.where(best < INF, best - o, F(-1.0)).astype(F)


def mesh_aabb(vertices):
    v = np.asarray(vertices, F)
    return v.min(axis=0), v.max(axis=0)


def sample_mesh(vertices, indices, particle_rad, mode, hits_per_ray=None):
    """The host arm's loop (salva_amd/csrc/sample.hip World::sample_host_shape; ray_sampling.rs:46-52, :109-126) fed with mesh_cast:
    all rays of an axis in rounds, impact = origin + toi, the next origin = origin + (toi + s / 10), entry and exit alternating.
    -> (indices, positions, N).  hits_per_ray (a list) receives the accepted hits of every ray."""
    mins, maxs = mesh_aabb(vertices)
    s, origin, coords = R.lattice(mins, maxs, particle_rad)
    N = [len(c) for c in coords]
    step = F(s / F(10.0))
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
            toi = mesh_cast(vertices, indices, org[live], i)
            keep = []
            for r, t in zip(live, toi):
                if not t >= 0:
                    continue
                count[r] += 1
                assert count[r] <= 64, "a ray with more than 64 accepted hits"
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


# ------------------------------------------------------------------------------------------------ the projection
def _dot(a, b):
    return ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])


def closest_on_triangles(vertices, indices, pts):
    """Ericson's ClosestPtPointTriangle of every point with every triangle, f32 -> (closest (n, T, 3), feature (n, T)): 0 1 2 = vertex
    a b c, 3 4 5 = edge ab ac bc, 6 = face."""
    v, tri = np.asarray(vertices, F), np.asarray(indices, np.int64)
    p = np.asarray(pts, F).reshape(-1, 1, 3)
    a, b, c = v[tri[:, 0]][None], v[tri[:, 1]][None], v[tri[:, 2]][None]
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = (d1 * d4) - (d3 * d2), (d5 * d2) - (d1 * d6), (d3 * d6) - (d5 * d4)
    with np.errstate(divide="ignore", invalid="ignore"):
        v_ab = (d1 / (d1 - d3))[..., None]
        w_ac = (d2 / (d2 - d6))[..., None]
        w_bc = ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None]
        denom = F(1.0) / ((va + vb) + vc)
        fv, fw = (vb * denom)[..., None], (vc * denom)[..., None]
        shape = np.broadcast_shapes(p.shape, a.shape)
        cases = [
            ((d1 <= 0) & (d2 <= 0), np.broadcast_to(a, shape), 0),
            ((d3 >= 0) & (d4 <= d3), np.broadcast_to(b, shape), 1),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + (ab * v_ab), 3),
            ((d6 >= 0) & (d5 <= d6), np.broadcast_to(c, shape), 2),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + (ac * w_ac), 4),
            ((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), b + ((c - b) * w_bc), 5),
        ]
        out = ((a + (ab * fv)) + (ac * fw)).astype(F)
    feat = np.full(out.shape[:2], 6, np.int64)
    for cond, point, code in reversed(cases):  # (the first case that holds wins)
        out = np.where(cond[..., None], point, out)
        feat = np.where(cond, code, feat)
    return out.astype(F), feat


def mesh_project(vertices, indices, normals, pts):
    """-> (closest points (n, 3) f32, is_inside (n,) bool): the smallest squared distance over all triangles, ties to the lowest
    triangle index; is_inside = dot(p - closest, pseudo-normal of the closest feature) <= 0, False without `normals`."""
    pts = np.asarray(pts, F).reshape(-1, 3)
    tri = np.asarray(indices, np.int64)
    out, inside = np.empty((len(pts), 3), F), np.zeros(len(pts), bool)
    for lo in range(0, len(pts), 512):  # (in blocks: n x T x 3 temporaries)
        p = pts[lo:lo + 512]
        close, feat = closest_on_triangles(vertices, indices, p)
        e = p[:, None, :] - close
        d = _dot(e, e)
        best = np.argmin(np.where(np.isnan(d), INF, d), axis=1)  # (the first of equal minima: the lowest triangle index)
        rows = np.arange(len(p))
        out[lo:lo + 512] = close[rows, best]
        if normals is None:
            continue
        for r in rows:
            t, f = best[r], feat[r, best[r]]
            if f == 6:
                n = normals["face"][t]
            elif f < 3:
                n = normals["vertex"][tri[t, f]]
            else:
                x, y = {3: (0, 1), 4: (0, 2), 5: (1, 2)}[int(f)]
                n = normals["edge"][(int(min(tri[t, x], tri[t, y])), int(max(tri[t, x], tri[t, y])))]
            dp = (p[r] - close[r, t]).astype(F)
            inside[lo + r] = ((dp[0] * n[0]) + (dp[1] * n[1])) + (dp[2] * n[2]) <= 0
    return out, inside
