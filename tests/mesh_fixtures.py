"""The meshes of the mesh tests, each a few lines of numpy: (a) the unit cube, (b) a concave L-prism turned so that
axis-parallel rays cross it twice, (c) a 5 x 5 and (d) a 9 x 9 height field, (e) a regular tetrahedron turned off the axes, and a
stack of 40 slabs for the hit bound.  -> (vertices f32, indices uint32, oriented)."""
import functools

import numpy as np

import mesh_reading as M

F = np.float32


def _rotation(axis_angle):
    """Rodrigues, f64."""
    w = np.asarray(axis_angle, np.float64)
    t = np.linalg.norm(w)
    k = w / t
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def box(lo, hi):
    """12 triangles wound counter-clockwise seen from outside; vertex x + 2 y + 4 z; every face's diagonal runs from its (-, -) to its
    (+, +) corner in the face's (j, k) coordinates, j = i + 1, k = i + 2 mod 3."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(hi if b >> a & 1 else lo)[a] for a in range(3)] for b in range(8)], F)
    tris = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        for side in (0, 1):
            c = [side << i | a << j | b << k for a, b in ((0, 0), (1, 0), (1, 1), (0, 1))]
            tris += [(c[0], c[1], c[2]), (c[0], c[2], c[3])] if side else [(c[0], c[2], c[1]), (c[0], c[3], c[2])]
    return v, np.asarray(tris, np.uint32)


@functools.lru_cache(maxsize=None)
def cube():
    v, t = box([-0.5] * 3, [0.5] * 3)
    return v, t, True


@functools.lru_cache(maxsize=None)
def l_prism():
    poly = np.array([(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2), (0, 1)], np.float64)
    cap = [(0, 1, 2), (0, 2, 3), (0, 3, 6), (6, 3, 4), (6, 4, 5)]
    n = len(poly)
    v = np.concatenate([np.c_[poly, np.full(n, -0.5)], np.c_[poly, np.full(n, 0.5)]])  # bottom k, top n + k
    tris = [(a + n, b + n, c + n) for a, b, c in cap] + [(a, c, b) for a, b, c in cap]
    for k in range(n):
        k1 = (k + 1) % n
        tris += [(k, k1, k1 + n), (k, k1 + n, k + n)]
    v = (v - [0.9, 0.9, 0.0]) * 0.23 @ _rotation([0.2, -0.1, np.pi / 4 + 0.05]).T
    return v.astype(F), np.asarray(tris, np.uint32), True


def _heights(n, seed):
    return np.random.default_rng(seed).random((n, n)).astype(F)


@functools.lru_cache(maxsize=None)
def heightfield5():
    v, t = M.heightfield_mesh(_heights(5, 11), (1.0, 0.3, 1.2))
    return v, t, False


@functools.lru_cache(maxsize=None)
def heightfield9():
    v, t = M.heightfield_mesh(_heights(9, 12), (1.1, 0.25, 0.9))
    return v, t, False


@functools.lru_cache(maxsize=None)
def tetrahedron():
    v = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], np.float64) * 0.17 @ _rotation([0.3, 0.5, -0.2]).T
    tris = []
    for skip in range(4):
        a, b, c = [x for x in range(4) if x != skip]
        if np.dot(np.cross(v[b] - v[a], v[c] - v[a]), v[a] - v[skip]) < 0:  # (outward: away from the fourth vertex)
            b, c = c, b
        tris.append((a, b, c))
    return v.astype(F), np.asarray(tris, np.uint32), True


@functools.lru_cache(maxsize=None)
def slabs(count=40):
    vs, ts = [], []
    for s in range(count):
        v, t = box([0.05 * s, -0.1, -0.1], [0.05 * s + 0.02, 0.1, 0.1])
        ts.append(t + 8 * s)
        vs.append(v)
    return np.concatenate(vs), np.concatenate(ts).astype(np.uint32), True


# name -> (fixture, a particle radius that gives at most 40 lattice lines per axis)
ALL = {"cube": (cube, 0.0625), "l_prism": (l_prism, 0.02), "heightfield5": (heightfield5, 0.02), "heightfield9": (heightfield9, 0.02),
       "tetrahedron": (tetrahedron, 0.01)}
