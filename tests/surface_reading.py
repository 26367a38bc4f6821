"""A numpy reading of the surface extractor's contract (include/salva_hip.h salva_hip_extract_surface): marching
tetrahedra on the Freudenthal split of every lattice cell.  Written from the header, not from the kernels: there is no case table
here - the triangles of a tetrahedron follow the header's three rules, and their orientation is decided geometrically, per triangle,
from the edge midpoints of the unit tetrahedron.  f32 wherever the contract says f32 (numpy rounds every f32 operation once and never
fuses), so that indices can be compared exactly and positions bit for bit.

Test infrastructure only."""
import itertools

import numpy as np

F32 = np.float32
AXES = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
PERMS = tuple(itertools.permutations(range(3)))  # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx
OFFSETS = tuple((ox, oy, oz) for ox in (0, 1) for oy in (0, 1) for oz in (0, 1))[1:]  # edge bit b = 4 ox + 2 oy + oz - 1


def edge_bit(o):
    return 4 * o[0] + 2 * o[1] + o[2] - 1


def tet_corners(t):
    """the four corners of tetrahedron t as offsets from the cell's min corner: v0 = 0, then one axis of the permutation at a time"""
    v = [np.zeros(3, int)]
    for axis in PERMS[t]:
        v.append(v[-1] + np.array(AXES[axis]))
    return v


def tet_triangles(t, m):
    """The triangles of tetrahedron t when the corners in bit mask m are inside: a list of triangles, each three tetrahedron edges
    (i, j) with i < j, in the header's order and oriented by the midpoint rule."""
    inside = [i for i in range(4) if (m >> i) & 1]
    outside = [i for i in range(4) if not (m >> i) & 1]

    def e(a, b):
        return (min(a, b), max(a, b))

    if len(inside) in (0, 4):
        return []
    if len(inside) == 1 or len(outside) == 1:
        a = inside[0] if len(inside) == 1 else outside[0]
        b, c, d = outside if len(inside) == 1 else inside
        tris = [[e(a, b), e(a, c), e(a, d)]]
    else:
        (a, b), (c, d) = inside, outside
        q = [e(a, c), e(a, d), e(b, d), e(b, c)]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    v = [c.astype(np.float64) for c in tet_corners(t)]
    towards = np.mean([v[i] for i in outside], axis=0) - np.mean([v[i] for i in inside], axis=0)
    out = []
    for tri in tris:
        p = [(v[i] + v[j]) / 2.0 for i, j in tri]
        normal = np.cross(p[1] - p[0], p[2] - p[0])
        s = float(normal @ towards)
        assert s != 0.0
        out.append(tri if s > 0.0 else [tri[0], tri[2], tri[1]])
    return out


def axis_nodes(origin, spacing, n):
    """origin + (float)i * spacing, product and sum each rounded in f32"""
    return (F32(origin) + (np.arange(n).astype(F32) * F32(spacing)).astype(F32)).astype(F32)


def extract(values, iso, origin, spacing):
    """values: (nx, ny, nz).  Returns (vertices (nv, 3) f32, triangles (nt, 3) uint32, the set of (tetrahedron, inside mask) pairs that
    occurred)."""
    f = np.ascontiguousarray(values, F32)
    nx, ny, nz = dims = f.shape
    assert min(dims) >= 2
    iso = F32(iso)
    inside = f >= iso
    n = f.size
    axes = [axis_nodes(np.asarray(origin, F32)[a], spacing, dims[a]) for a in range(3)]
    node = np.arange(n).reshape(dims)

    def lower(o):  # the nodes p with p + o in the lattice, and those p + o
        a = tuple(slice(0, dims[k] - o[k]) for k in range(3))
        b = tuple(slice(o[k], dims[k]) for k in range(3))
        return a, b

    # edges: node p owns the edge to p + o; it carries a vertex iff exactly one end is inside
    has = np.zeros((7,) + dims, bool)
    for o in OFFSETS:
        a, b = lower(o)
        has[(edge_bit(o),) + a] = inside[a] != inside[b]
    mask = sum(has[b].astype(np.int64) << b for b in range(7)).reshape(n)
    count = has.reshape(7, n).sum(axis=0)
    first = np.concatenate([[0], np.cumsum(count)])  # by owner node ascending ...
    nv = int(first[-1])
    below = np.stack([has.reshape(7, n)[:b].sum(axis=0) for b in range(7)])  # ... then edge bit ascending
    index = first[:n][None, :] + below  # (7, n): the vertex of (edge bit, node), where there is one
    vertices = np.zeros((nv, 3), F32)
    for o in OFFSETS:
        b = edge_bit(o)
        a_, b_ = lower(o)
        sel = has[(b,) + a_]
        fa, fb = f[a_][sel], f[b_][sel]
        with np.errstate(all="ignore"):
            t = ((iso - fa).astype(F32) / (fb - fa).astype(F32)).astype(F32)
        rows = index[b].reshape(dims)[a_][sel]
        grids = np.meshgrid(*[np.arange(dims[k] - o[k]) for k in range(3)], indexing="ij")
        for k in range(3):
            i = grids[k][sel]
            pa, pb = axes[k][i], axes[k][i + o[k]]
            with np.errstate(all="ignore"):
                vertices[rows, k] = (pa + (t * (pb - pa).astype(F32)).astype(F32)).astype(F32)
    # cells: min corner c with c + (1, 1, 1) in the lattice
    cell = node[:-1, :-1, :-1]
    keys, tris, seen = [], [], set()
    for t in range(6):
        v = tet_corners(t)
        m = np.zeros(cell.shape, int)
        for i in range(4):
            m |= inside[v[i][0]:nx - 1 + v[i][0], v[i][1]:ny - 1 + v[i][1], v[i][2]:nz - 1 + v[i][2]].astype(int) << i
        for case in range(1, 15):
            sel = m == case
            if not sel.any():
                continue
            seen.add((t, case))
            cells = cell[sel]
            for k, tri in enumerate(tet_triangles(t, case)):
                cols = []
                for i, j in tri:
                    owner = cells + (v[i][0] * ny + v[i][1]) * nz + v[i][2]
                    bit = edge_bit(tuple(v[j] - v[i]))
                    assert ((mask[owner] >> bit) & 1).all()
                    cols.append(index[bit, owner])
                tris.append(np.stack(cols, axis=1))
                keys.append(np.stack([cells, np.full(len(cells), t), np.full(len(cells), k)], axis=1))
    if not tris:
        return vertices, np.zeros((0, 3), np.uint32), seen
    tris, keys = np.concatenate(tris), np.concatenate(keys)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))  # by cell, then tetrahedron, then the order of the rules
    return vertices, tris[order].astype(np.uint32), seen


# ------------------------------------------------------------------------------------------------ what the tests ask of a mesh
def directed_edges(triangles):
    t = np.asarray(triangles, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def edge_report(triangles):
    """(no directed edge occurs twice, the directed edges whose reverse is absent)"""
    e = directed_edges(triangles)
    big = int(e.max()) + 1 if len(e) else 1
    key = e[:, 0] * big + e[:, 1]
    unique = len(np.unique(key)) == len(key)
    open_ = e[~np.isin(e[:, 1] * big + e[:, 0], key)]
    return unique, open_


def euler_characteristic(nv, triangles):
    e = np.sort(directed_edges(triangles), axis=1)
    return nv - len(np.unique(e, axis=0)) + len(triangles)


def signed_volume(vertices, triangles):
    p = np.asarray(vertices, np.float64)[np.asarray(triangles, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def area(vertices, triangles):
    p = np.asarray(vertices, np.float64)[np.asarray(triangles, np.int64)]
    return float(np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).sum() / 2.0)


# ------------------------------------------------------------------------------------------------ the lattices of the tests
LATTICE_ORIGIN = (-0.3, 0.1, 0.2)
LATTICE_SPACING = 0.05
LINEAR_N = (0.3, -0.5, 0.81)
LINEAR_ISO = 0.1  # n . x runs from -0.10 to 0.27 over the lattice


def random_lattice():
    return np.random.default_rng(0).uniform(0, 1, (7, 6, 5)).astype(F32)


def linear_lattice():
    """f = n . x at the nodes of the 7 x 6 x 5 lattice at LATTICE_ORIGIN, spacing LATTICE_SPACING (f64, rounded once to f32)"""
    axes = [axis_nodes(LATTICE_ORIGIN[a], LATTICE_SPACING, d).astype(np.float64) for a, d in enumerate((7, 6, 5))]
    gx, gy, gz = np.meshgrid(*axes, indexing="ij")
    return (LINEAR_N[0] * gx + LINEAR_N[1] * gy + LINEAR_N[2] * gz).astype(F32)
