"""An independent numpy reading of the compound collider of DESIGN.md §17: the compound's box, the projection of a point on it
and its solid distance.  f32 operation by operation, a brute force over ALL parts — no per-part boxes, no pruning — built from the
per-shape callbacks the host-shape tests already use (tests/test_host_shape_gpu.py, tests/dcs_cloud.py) and the mesh reading
(tests/mesh_reading.py).  What salva_amd/csrc/compound.h is compared with bit for bit.

A part is (shape, translation, rotation): `shape` what salva_amd.coupling.make_shape takes, or ("mesh", vertices, indices, oriented);
the pose places the part in the compound's frame.  A `body` (anything with .translation and .rotation) places the compound."""
from types import SimpleNamespace

import numpy as np

import dcs_cloud as D
import mesh_reading as M
from test_host_shape_gpu import quat_rot, to_local, to_world

F = np.float32
INF = F(np.inf)
IDENTITY = SimpleNamespace(translation=np.zeros(3, F), rotation=F([0, 0, 0, 1]))


def pose(translation, rotation):
    return SimpleNamespace(translation=np.asarray(translation, F), rotation=np.asarray(rotation, F))


def _rotation_abs(q):
    """|UnitQuaternion::to_rotation_matrix|, f32 (the matrix of test_host_shape_gpu.cuboid_callbacks)."""
    i, j, k, w = (F(x) for x in q)
    ww, ii, jj, kk = w * w, i * i, j * j, k * k
    ij, wk, wj, ik, jk, wi = i * j * F(2), w * k * F(2), w * j * F(2), i * k * F(2), j * k * F(2), w * i * F(2)
    return np.abs(np.array([[ww + ii - jj - kk, ij - wk, wj + ik], [wk + ij, ww - ii + jj - kk, jk - wi], [ik - wj, wi + jk, ww - ii - jj + kk]], F))


def transform_by(lo, hi, p):
    """parry's Aabb::transform_by: the box's centre posed, -+ |R| half_extents."""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    centre, he = ((lo + hi) * F(0.5)).astype(F), ((hi - lo) * F(0.5)).astype(F)
    m = _rotation_abs(p.rotation)
    ext = ((m[:, 0] * he[0] + m[:, 1] * he[1]) + m[:, 2] * he[2]).astype(F)
    c = to_world(p, centre[None])[0]
    return (c - ext).astype(F), (c + ext).astype(F)


def part_aabb(part):
    """parry's part.compute_aabb(part_pos) in the compound's frame."""
    shape, t, q = part
    p = pose(t, q)
    if shape[0] == "mesh":
        return transform_by(*M.mesh_aabb(shape[1]), p)
    if shape[0] == "ball":
        ext = np.full(3, F(shape[1]), F)
    elif shape[0] == "capsule":  # the posed segment ends are t -+ q * (0, hh, 0): extent = |q * b| + radius
        ext = (np.abs(quat_rot(p.rotation, np.array([[0, shape[1], 0]], F))[0]) + F(shape[2])).astype(F)
    else:
        he = F(shape[1]) if shape[0] == "cuboid" else F([shape[2], shape[1], shape[2]])
        m = _rotation_abs(p.rotation)
        ext = ((m[:, 0] * he[0] + m[:, 1] * he[1]) + m[:, 2] * he[2]).astype(F)
    return (p.translation - ext).astype(F), (p.translation + ext).astype(F)


def local_aabb(parts):
    """The merge of the parts' boxes."""
    boxes = [part_aabb(p) for p in parts]
    return np.min([b[0] for b in boxes], axis=0).astype(F), np.max([b[1] for b in boxes], axis=0).astype(F)


def aabb(parts, body):
    """`compound.compute_aabb(body pose)` as the device takes it: the local box through transform_by."""
    return transform_by(*local_aabb(parts), body)


def _normals(shape):
    return M.pseudo_normals(shape[1], shape[2]) if shape[3] else None


def part_project(part, l, normals=None):
    """The projection of compound-frame points on one part's boundary, in the compound's frame, and is_inside."""
    shape, t, q = part
    p = pose(t, q)
    if shape[0] == "mesh":
        proj, inside = M.mesh_project(shape[1], shape[2], normals if normals is not None else _normals(shape), to_local(p, l))
        return to_world(p, proj), inside
    with np.errstate(divide="ignore", invalid="ignore"):
        return D.callbacks(D.Collider("part", shape, p))[1](l)


def project_local(parts, l, winners=None):
    """Every part in index order; the smallest ((dx dx + dy dy) + dz dz) of l - c_k wins, a tie stays with the lower index."""
    l = np.asarray(l, F).reshape(-1, 3)
    best = np.full(len(l), INF, F)
    out, inside, who = l.copy(), np.zeros(len(l), bool), np.full(len(l), -1)
    for k, part in enumerate(parts):
        c, ins = part_project(part, l)
        d = (l - c).astype(F)
        d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)
        with np.errstate(invalid="ignore"):
            win = d2 < best
        best = np.where(win, d2, best)
        out[win], inside[win], who[win] = c[win], np.asarray(ins, bool)[win], k
    if winners is not None:
        winners.append(who)
    return out, inside


def project(parts, body, pts, winners=None):
    """project_point_and_get_feature(body pose, pt) with solid = false -> (world projections, is_inside)."""
    proj, inside = project_local(parts, to_local(body, np.asarray(pts, F).reshape(-1, 3)), winners)
    return to_world(body, proj), inside


def callbacks(parts, body, log=None):
    """(aabb, project) for HostShapeSampling; `log` receives the number of points inside per call."""
    def project_cb(pts):
        proj, inside = project(parts, body, pts)
        if log is not None:
            log.append(int(inside.sum()))
        return proj, inside

    return (lambda: aabb(parts, body)), project_cb


def shape_distance(shape, l):
    """distance_to_point(identity, l, solid = true) of a built-in shape, as world_query.hip's shape_solid_distance computes it."""
    x, y, z = l[:, 0], l[:, 1], l[:, 2]
    if shape[0] == "ball":
        return np.maximum(np.sqrt((x * x + y * y) + z * z) - F(shape[1]), F(0)).astype(F)
    if shape[0] == "capsule":
        hh, r = F(shape[1]), F(shape[2])
        ey = (y - np.minimum(np.maximum(y, -hh), hh)).astype(F)
        return np.maximum(np.sqrt((x * x + ey * ey) + z * z) - r, F(0)).astype(F)
    if shape[0] == "cylinder":
        hh, r = F(shape[1]), F(shape[2])
        ey, er = np.maximum(np.abs(y) - hh, F(0)).astype(F), np.maximum(np.sqrt(x * x + z * z) - r, F(0)).astype(F)
        return np.sqrt(ey * ey + er * er).astype(F)
    he = F(shape[1])
    d = np.maximum(np.abs(l) - he, F(0)).astype(F)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)


def mesh_distance(shape, l):
    """An oriented mesh: 0 inside, the distance to the closest point outside."""
    assert shape[3], "a mesh that is not oriented has no solid distance"
    proj, inside = M.mesh_project(shape[1], shape[2], _normals(shape), l)
    d = (l - proj).astype(F)
    return np.where(inside, F(0), np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])).astype(F)


def distance(parts, body, pts):
    """The compound's solid distance: the smallest of its parts', each in the part's frame."""
    l = to_local(body, np.asarray(pts, F).reshape(-1, 3))
    out = np.full(len(l), INF, F)
    for shape, t, q in parts:
        lk = to_local(pose(t, q), l)
        out = np.fmin(out, mesh_distance(shape, lk) if shape[0] == "mesh" else shape_distance(shape, lk))
    return out


def to_compound(parts):
    """The same parts as a salva_amd.sampling.Compound."""
    from salva_amd import sampling

    return sampling.Compound([(sampling.Mesh(s[1], s[2], oriented=s[3]) if s[0] == "mesh" else s, t, q) for s, t, q in parts])
