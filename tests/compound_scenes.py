"""The compounds of the compound tests, shared by tests/test_compound_cpu.py and tests/test_compound_gpu.py.  Parts
are what tests/compound_reading.py takes: (shape, translation, rotation)."""
import numpy as np

import mesh_fixtures as X
from salva_amd import scenes

F = np.float32
R = 0.025
H = F(F(R) * F(2.0)) * F(2.0)          # particle radius * smoothing factor * 2 (liquid_world.rs:44)
REACH = F(H + F(H * F(0.5)))           # h + prediction (dcs.hip dcs_params)
EPS = F(np.finfo(np.float32).eps)
ID = F([0, 0, 0, 1])


def quat(axis):
    return scenes.quat_from_scaled_axis(axis).astype(F)


def tetra(scale=0.11 / 0.17):
    v, t, _ = X.tetrahedron()
    return ("mesh", (v * F(scale)).astype(F), t, True)


def cube_mesh(he):
    v, t, _ = X.cube()
    return ("mesh", (v * (F(2) * F(he))).astype(F), t, True)


def body_compound():
    """A rotated cuboid, a capsule and an oriented tetrahedron that overlap: what rides on the moving, spinning body."""
    return [(("cuboid", (0.10, 0.035, 0.08)), F([0.0, -0.02, 0.0]), quat((0.2, -0.3, 0.4))),
            (("capsule", 0.07, 0.045), F([0.06, 0.03, -0.01]), quat((-0.5, 0.2, 0.9))),
            (tetra(), F([-0.05, 0.04, 0.03]), quat((0.1, 0.6, -0.2)))]


def slab_compound():
    """Two overlapping slabs and a cylinder standing on them: what the tilted, resting body carries."""
    return [(("cuboid", (0.17, 0.04, 0.22)), F([-0.14, 0.0, 0.0]), ID),
            (("cuboid", (0.17, 0.04, 0.22)), F([0.14, 0.0, 0.0]), quat((0.0, 0.3, 0.0))),
            (("cylinder", 0.05, 0.06), F([0.02, 0.06, 0.03]), quat((0.2, 0.0, -0.1)))]


def deep_in_a_near_b():
    """A big ball A and a small ball B just beside the test point, which lies deep inside A and outside B."""
    parts = [(("ball", 0.25), F([0.0, 0.0, 0.0]), ID), (("ball", 0.03125), F([0.0625, 0.0, 0.0]), ID)]
    point = F([[0.0, 0.0, 0.0]]) + F([0.015625, 0.0, 0.0])   # 0.234 inside A; 0.0156 outside B's surface
    return parts, point


def mirrored_balls():
    """Two identical balls mirrored in the plane x = 0 (dyadic sizes, identity rotations) and points ON that plane: exact ties."""
    parts = [(("ball", 0.125), F([-0.0625, 0.0, 0.0]), ID), (("ball", 0.125), F([0.0625, 0.0, 0.0]), ID)]
    points = F([[0.0, 0.25, 0.0], [0.0, 0.0625, 0.03125], [0.0, -0.125, 0.125], [0.0, 0.03125, -0.015625]])
    return parts, points


def far_apart():
    """Five parts whose boxes are far from each other: the walk leaves most of them out for most points."""
    return [(("ball", 0.06), F([-0.45, 0.0, 0.0]), ID),
            (("cuboid", (0.05, 0.07, 0.04)), F([0.0, 0.4, 0.0]), quat((0.3, 0.2, -0.4))),
            (("capsule", 0.06, 0.04), F([0.45, 0.0, 0.1]), quat((0.0, 0.0, 1.2))),
            (("cylinder", 0.05, 0.06), F([0.0, -0.4, -0.1]), quat((0.7, 0.0, 0.1))),
            (("ball", 0.05), F([0.05, 0.0, 0.45]), ID)]


def lattice_cloud(centre, count, seed=21):
    """The `count` points of a jittered 2 R lattice nearest to `centre`."""
    n = 12
    pos = scenes.jitter(scenes.cube_fluid_positions(n, n, n, R), 0.2 * R, seed=seed) + F(centre)
    order = np.argsort(np.linalg.norm(pos.astype(np.float64) - np.asarray(centre, np.float64), axis=1), kind="stable")
    return pos[order[:count]].astype(F)


def emits(pred, proj, inside):
    """fluids_pipeline.rs:219-243 after the projection, f32: which points emit a boundary particle."""
    d = (pred - proj).astype(F)
    sq = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)
    with np.errstate(invalid="ignore"):
        far = (sq > EPS * EPS) & ~np.asarray(inside, bool) & (np.sqrt(sq) > REACH)
    return ~far
