"""The compound collider of DESIGN.md §17 without a GPU: the numpy reading (tests/compound_reading.py) against an f64 brute force,
against a part's own reading, on the two cases the reading of parry's Compound projection turns on — inside A but nearer to B, and
an exact tie — and the library's `__host__ __device__` walk with its box pruning against the walk over all parts (a stand-alone host
program, tests/compound_walk_check.hip)."""
import os
import re
import subprocess

import numpy as np

import compound_reading as CR
import compound_scenes as CS
import dcs_cloud as D
from test_host_shape_gpu import to_local
from test_kernel_resources import CSRC, HIPCC, pytestmark  # noqa: F401

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))


def _f64_parts(parts, body, pts):
    """Per part, in f64: the nearest surface point (world) and inside, from dcs_cloud.classify on the part's composed pose."""
    Rb, tb = D.rotation_matrix(body.rotation), body.translation.astype(np.float64)
    out = []
    for shape, t, q in parts:
        Rk = Rb @ D.rotation_matrix(q)
        tk = Rb @ np.asarray(t, np.float64) + tb
        l = (np.asarray(pts, np.float64) - tk) @ Rk
        c = D.Collider("part", shape, CR.IDENTITY)
        with np.errstate(divide="ignore", invalid="ignore"):
            _, inside, near = D._classify(c, l)
        out.append((near @ Rk.T + tk, inside))
    return out


def test_reading_matches_an_f64_brute_force():
    parts = [p for p in CS.body_compound() if p[0][0] != "mesh"] + CS.slab_compound()
    body = CR.pose([0.08, 0.30, 0.05], CS.quat((0.4, -0.3, 0.2)))
    rng = np.random.default_rng(3)
    lo, hi = CR.aabb(parts, body)
    pts = (lo - 0.1 + rng.random((4000, 3)) * (hi - lo + 0.2)).astype(F)
    winners = []
    proj, inside = CR.project(parts, body, pts, winners)
    per_part = _f64_parts(parts, body, pts)
    d = np.stack([np.linalg.norm(pts.astype(np.float64) - near, axis=1) for near, _ in per_part], axis=1)
    order = np.sort(d, axis=1)
    clear = order[:, 1] - order[:, 0] > 1e-5   # the winner is not a matter of rounding
    best = d.argmin(axis=1)
    assert clear.sum() > 3500
    assert np.array_equal(winners[0][clear], best[clear])
    near = np.stack([per_part[k][0][i] for i, k in enumerate(best)])
    ins = np.array([per_part[k][1][i] for i, k in enumerate(best)])
    assert np.abs(proj[clear] - near[clear]).max() < 2e-6
    off = np.abs(order[:, 0]) > 1e-5           # not on the surface, where is_inside is a matter of rounding
    assert np.array_equal(inside[clear & off], ins[clear & off])
    assert 100 < inside.sum() < 3900
    # the solid distance: 0 inside some part, the distance to the nearest part otherwise
    dist = CR.distance(parts, body, pts)
    inside_any = np.stack([i for _, i in per_part], axis=1).any(axis=1)
    want = np.where(inside_any, 0.0, order[:, 0])
    assert np.abs(dist - want)[off].max() < 2e-6


def test_the_box_is_the_merge_of_the_parts_boxes_posed():
    """Against f64: every part's box from its own extent (dcs_cloud.half_extent), merged, then Aabb::transform_by."""
    parts = CS.body_compound()[:2] + CS.slab_compound()
    lo, hi = CR.local_aabb(parts)
    boxes = []
    for shape, t, q in parts:
        ext = D.half_extent(D.Collider("part", shape, CR.pose(t, q)))
        boxes.append((np.asarray(t, np.float64) - ext, np.asarray(t, np.float64) + ext))
    assert np.abs(lo - np.min([b[0] for b in boxes], axis=0)).max() < 1e-6 and np.abs(hi - np.max([b[1] for b in boxes], axis=0)).max() < 1e-6
    body = CR.pose([0.3, -0.2, 0.1], CS.quat((0.5, 0.1, -0.7)))
    wlo, whi = CR.aabb(parts, body)
    Rm = D.rotation_matrix(body.rotation)
    c, he = (lo.astype(np.float64) + hi) / 2, (hi.astype(np.float64) - lo) / 2
    assert np.abs(wlo - (Rm @ c + body.translation - np.abs(Rm) @ he)).max() < 1e-6
    assert np.abs(whi - (Rm @ c + body.translation + np.abs(Rm) @ he)).max() < 1e-6
    # a mesh part: its vertices, posed, lie in its box
    shape, t, q = CS.body_compound()[2]
    mlo, mhi = CR.part_aabb((shape, t, q))
    v = shape[1].astype(np.float64) @ D.rotation_matrix(q).T + t
    assert (v >= mlo - 1e-6).all() and (v <= mhi + 1e-6).all()


def test_a_one_part_compound_is_the_part():
    rng = np.random.default_rng(4)
    body = CR.pose([0.05, -0.02, 0.03], CS.quat((0.3, -0.2, 0.5)))
    pts = ((rng.random((500, 3)) - 0.5) * 0.8).astype(F)
    for shape in (("ball", 0.17), ("cuboid", (0.22, 0.12, 0.17)), ("capsule", 0.16, 0.11), ("cylinder", 0.09, 0.21)):
        with np.errstate(divide="ignore", invalid="ignore"):
            want, want_in = D.callbacks(D.Collider("x", shape, body))[1](pts)
        got, got_in = CR.project([(shape, np.zeros(3, F), CS.ID)], body, pts)
        # (an identity part pose is not arithmetic-free: -0 becomes +0, which compares equal)
        assert np.array_equal(got, want) and np.array_equal(got_in, want_in), shape
    shape = CS.tetra()
    import mesh_reading as M
    want, want_in = M.mesh_project(shape[1], shape[2], M.pseudo_normals(shape[1], shape[2]), to_local(body, pts))
    got, got_in = CR.project_local([(shape, np.zeros(3, F), CS.ID)], to_local(body, pts))
    assert np.array_equal(got, want) and np.array_equal(got_in, want_in)


def test_deep_inside_a_but_nearer_to_b_is_outside_on_b():
    parts, point = CS.deep_in_a_near_b()
    winners = []
    proj, inside = CR.project(parts, CR.IDENTITY, point, winners)
    assert winners[0][0] == 1 and not inside[0]
    assert np.array_equal(proj[0], F([0.03125, 0.0, 0.0]))
    assert CR.part_project(parts[0], point)[1][0], "the point does lie inside A"
    assert CR.distance(parts, CR.IDENTITY, point)[0] == 0.0  # (the solid distance is another matter: inside A)


def test_an_exact_tie_goes_to_part_0():
    parts, points = CS.mirrored_balls()
    c0, _ = CR.part_project(parts[0], points)
    c1, _ = CR.part_project(parts[1], points)
    d0, d1 = (points - c0).astype(F), (points - c1).astype(F)
    sq = lambda d: ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)  # noqa: E731
    assert np.array_equal(sq(d0), sq(d1)) and (c0[:, 0] == -c1[:, 0]).all() and (c0[:, 0] != 0).all(), "the scene is not an exact tie"
    winners = []
    proj, _ = CR.project(parts, CR.IDENTITY, points, winners)
    assert (winners[0] == 0).all() and np.array_equal(proj, c0)
    swapped, _ = CR.project(parts[::-1], CR.IDENTITY, points)
    assert np.array_equal(swapped, c1)


def test_pruned_walk_equals_the_walk_over_all_parts(hip_lib, tmp_path):
    exe = str(tmp_path / "compound_walk_check")
    build = subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + CSRC, os.path.join(HERE, "compound_walk_check.hip"),
                            "-o", exe, "-L" + CSRC, "-lsalva_hip", "-Wl,-rpath," + CSRC], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    m = re.search(r"part visits: (\d+), .*: (\d+); differences: (\d+)", run.stdout)
    assert run.returncode == 0 and m and int(m.group(3)) == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert int(m.group(2)) > int(m.group(1)) // 8, "hardly any part was left out: the pruning was not exercised"
