"""The general-direction ray casts behind the ray sampler of a compound (salva_amd/csrc/raycast.h, DESIGN.md §17 "Ray sampling")
without a GPU: the library's `__host__ __device__` casts run by a stand-alone host program (tests/compound_cast_check.hip) — pruned
walks against walks over everything, the casts against the numpy reading (tests/compound_cast_reading.py) bit for bit, even
crossings on closed meshes — and the reading against an independent f64 evaluation."""
import os
import re
import subprocess

import numpy as np
import pytest

import compound_cast_reading as CC
import compound_reading as CR
import compound_scenes as CS
import mesh_fixtures as X
from test_kernel_resources import CSRC, HIPCC, pytestmark  # noqa: F401

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
KIND = {"ball": 1, "cuboid": 2, "capsule": 3, "cylinder": 4, "mesh": 5}
ROTATIONS = ((0.31, -0.52, 0.23), (-0.7, 0.4, 1.1), (1.3, 0.9, -0.45))   # three generic rotations (scaled axes)


def _hex(x):
    return "%08x" % int(np.asarray(x, F).reshape(1).view(np.uint32)[0])


class Job:
    """The text compound_cast_check reads: meshes, compounds and jobs, floats as hex bit patterns."""

    def __init__(self):
        self.lines, self.nmesh, self.ncompound = [], 0, 0

    def mesh(self, v, t):
        v, t = np.asarray(v, F).reshape(-1, 3), np.asarray(t, np.uint32).reshape(-1, 3)
        self.lines.append("mesh %d %d" % (len(v), len(t)))
        self.lines += [" ".join(_hex(x) for x in row) for row in v] + [" ".join(str(int(x)) for x in row) for row in t]
        self.nmesh += 1
        return self.nmesh - 1

    def compound(self, parts):
        rows = []
        for shape, t, q in parts:
            m = self.mesh(shape[1], shape[2]) if shape[0] == "mesh" else -1
            p = [0, 0, 0] if shape[0] == "mesh" else (list(shape[1]) if shape[0] == "cuboid" else list(shape[1:]) + [0] * (4 - len(shape)))
            rows.append(" ".join([str(KIND[shape[0]])] + [_hex(x) for x in p] + [str(m)] + [_hex(x) for x in t] + [_hex(x) for x in q]))
        self.lines += ["compound %d" % len(parts)] + rows
        self.ncompound += 1
        return self.ncompound - 1

    def write(self, path):
        with open(path, "w") as f:
            f.write("\n".join(self.lines) + "\n")


@pytest.fixture(scope="module")
def check(hip_lib, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("compound_cast") / "compound_cast_check")
    build = subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + CSRC, os.path.join(HERE, "compound_cast_check.hip"),
                            "-o", exe, "-L" + CSRC, "-lsalva_hip", "-Wl,-rpath," + CSRC], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]

    def run(job, tmp_path):
        path = str(tmp_path / "job.txt")
        job.write(path)
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout

    return run


def generic_rays(parts, n, seed):
    """Random unit directions; origins in the compound's box and a fifth beyond, half of them aimed at a part's centre."""
    rng = np.random.default_rng(seed)
    lo, hi = CR.local_aabb(parts)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(F)
    o = (lo - 0.2 * (hi - lo) + rng.random((n, 3)) * 1.4 * (hi - lo)).astype(F)
    aim = rng.integers(0, len(parts), n)
    centre = np.stack([np.asarray(parts[k][1], np.float64) for k in aim]) + (rng.random((n, 3)) - 0.5) * 0.04
    back = (0.1 + 0.5 * rng.random(n))[:, None]
    aimed = (np.arange(n) % 2 == 0)[:, None]
    return np.where(aimed, centre - back * d, o).astype(F), d


def kinds_compound():
    """Every kind at a generic pose, with two concave / boxy meshes among them."""
    lp, cube = X.l_prism(), X.cube()
    return [(("ball", 0.11), F([0.3, 0.1, -0.2]), CS.quat((0.2, 0.1, -0.3))),
            (("cuboid", (0.12, 0.05, 0.2)), F([-0.2, 0.05, 0.1]), CS.quat(ROTATIONS[0])),
            (("capsule", 0.15, 0.06), F([0.0, -0.3, 0.2]), CS.quat(ROTATIONS[1])),
            (("cylinder", 0.04, 0.14), F([0.1, 0.3, 0.3]), CS.quat(ROTATIONS[2])),
            (("mesh", lp[0], lp[1], True), F([-0.1, -0.1, -0.3]), CS.quat((0.5, -0.2, 0.3))),
            (("mesh", (cube[0] * F(0.2)).astype(F), cube[1], True), F([0.35, -0.25, 0.15]), CS.quat((-0.4, 0.6, 0.2)))]


# ------------------------------------------------------------------------------------------------ (a) pruning is exact
def test_pruned_walks_equal_the_walks_over_everything(check, tmp_path):
    job = Job()
    for fixture in (lambda: X.slabs(40), X.heightfield9, X.l_prism):
        v, t, _ = fixture()
        job.lines.append("prune_mesh %d 4000" % job.mesh(v, t))
    for scene in list(CC.SCENES.values()) + [kinds_compound]:
        job.lines.append("prune_compound %d 4000" % job.compound(scene()))
    out = check(job, tmp_path)
    print(out)
    meshes = re.findall(r"prune_mesh (\d+) casts (\d+) hits (\d+) depth (\d+) differences (\d+)", out)
    compounds = re.findall(r"prune_compound (\d+) casts (\d+) hits (\d+) visits (\d+) pruned (\d+) differences (\d+)", out)
    assert len(meshes) == 3 and len(compounds) == 5
    for m in meshes:
        assert int(m[4]) == 0 and int(m[2]) > 1000, m
    assert max(int(m[3]) for m in meshes) >= 7
    for c in compounds:
        assert int(c[5]) == 0 and int(c[2]) > 1000, c
        assert int(c[4]) > int(c[3]) // 8, "hardly any part was left out: the pruning was not exercised"


# ------------------------------------------------------------------------------------------------ (b) the C++ casts are the reading
def test_casts_equal_the_reading_bit_for_bit(check, tmp_path):
    job, want = Job(), []
    for seed, scene in enumerate(list(CC.SCENES.values()) + [kinds_compound]):
        parts = scene()
        o, d = generic_rays(parts, 1500, 40 + seed)
        # the sampler's own rays among them: axis-parallel, where a slab runs beside the ray
        d[::10] = CC.axis_dirs(len(d[::10]), seed % 3)
        job.lines.append("cast %d %d" % (job.compound(parts), len(o)))
        job.lines += [" ".join(_hex(x) for x in np.r_[a, b]) for a, b in zip(o, d)]
        winners = []
        want.append(CC.compound_cast(parts, o, d, winners))
        hit = winners[0] >= 0
        print(scene.__name__, "hits", int(hit.sum()), "of", len(o), "parts that win", sorted(set(winners[0][hit].tolist())))
        assert 150 < hit.sum() < len(o) - 150
        if scene is kinds_compound:
            assert set(winners[0][hit].tolist()) == set(range(6)), "some kind never wins a ray"
    got = np.array([int(x, 16) for x in re.findall(r"toi ([0-9a-f]{8})", check(job, tmp_path))], np.uint32)
    want = np.concatenate(want).view(np.uint32)
    assert len(got) == len(want)
    diff = np.nonzero(got != want)[0]
    assert len(diff) == 0, (len(diff), diff[:10], got[diff[:10]].view(F), want[diff[:10]].view(F))


# ------------------------------------------------------------------------------------------------ (c) closed meshes, even crossings
def test_closed_meshes_have_even_crossings(check, tmp_path):
    job, names = Job(), []
    for fixture, rad in ((X.cube, 0.02), (X.tetrahedron, 0.005), (X.l_prism, 0.01)):
        v, t, oriented = fixture()
        assert oriented
        for axis in ROTATIONS:
            c = job.compound([(("mesh", v, t, True), F([0.03, -0.02, 0.05]), CS.quat(axis))])
            job.lines.append("parity %d %s" % (c, _hex(rad)))
            names.append((fixture.__name__, axis))
    out = check(job, tmp_path)
    print(out)
    rows = re.findall(r"parity (\d+) rays (\d+) hits (\d+) odd (\d+)", out)
    assert len(rows) == 9
    for row, name in zip(rows, names):
        assert int(row[1]) > 3000 and int(row[2]) > 1000, (name, row)
        assert int(row[3]) == 0, (name, row)


# ------------------------------------------------------------------------------------------------ the reading against f64
def _winding(v, tri, p):
    """The winding number of a closed mesh about points, f64 (Van Oosterom & Strackee's solid angles)."""
    v = np.asarray(v, np.float64)
    a, b, c = (v[tri[:, k]][None] - p[:, None, :] for k in range(3))
    la, lb, lc = (np.linalg.norm(x, axis=2) for x in (a, b, c))
    det = np.einsum("ijk,ijk->ij", a, np.cross(b, c))
    den = la * lb * lc + np.einsum("ijk,ijk->ij", a, b) * lc + np.einsum("ijk,ijk->ij", b, c) * la + np.einsum("ijk,ijk->ij", c, a) * lb
    return np.arctan2(det, den).sum(axis=1) / (2.0 * np.pi)


def _signed_depth(part, p):
    """f64 points in the compound's frame -> depth inside the part (negative: the distance outside).  The distance is that to
    compound_reading.part_project's projection; a mesh part's side is its winding number's."""
    proj, inside = CR.part_project(part, p.astype(F))
    dist = np.linalg.norm(p - proj.astype(np.float64), axis=1)
    if part[0][0] == "mesh":
        from test_host_shape_gpu import to_local
        inside = np.abs(_winding(part[0][1], np.asarray(part[0][2], np.int64), to_local(CR.pose(part[1], part[2]), p.astype(F)).astype(np.float64))) > 0.5
    return np.where(inside, dist, -dist)


@pytest.mark.parametrize("name", list(CC.SCENES))
def test_reading_against_an_f64_evaluation(name):
    """Per part and ray: a hit lies on the part's boundary within 2^-18 of the largest coordinate of the compound's local box, and up
    to the reported crossing (for a miss: all the way) 4096 f64 samples stay on the origin's side of the boundary within the same
    bound.  Rays that graze — whose deepest sample inside the part, or nearest sample outside it, lies within the bound of the
    boundary, or that start that close to it — are left out; observed with these seeds: none of the 6483 (ray, part) pairs that reach
    a part's box in the four scenes (1500 rays each), against the 1 % of the rays allowed.  The worst hits observed lie 1.1e-7
    (body_compound; its bound is 1.0e-6) and 1.7e-7 (the ring; 1.7e-6) off the boundary."""
    parts = CC.SCENES[name]()
    lo, hi = CR.local_aabb(parts)
    bound = 2.0 ** -18 * float(max(np.abs(lo).max(), np.abs(hi).max()))
    o, d = generic_rays(parts, 1500, 7 + list(CC.SCENES).index(name))
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    pairs = grazing = hits = worst_hit = worst_side = 0
    for part in parts:
        t = CC.part_cast(part, o, d).astype(np.float64)
        blo, bhi = (x.astype(np.float64) for x in CR.part_aabb(part))
        # the stretch of the ray in the part's box (loosened by a hundred bounds): outside it the ray is outside the part
        with np.errstate(divide="ignore", invalid="ignore"):
            u, w = (blo - 100 * bound - o64) / d64, (bhi + 100 * bound - o64) / d64
        t0, t1 = np.maximum(np.minimum(u, w).max(axis=1), 0.0), np.maximum(u, w).min(axis=1)
        reach = t0 < t1
        assert (np.isinf(t) | reach).all(), "a hit outside the part's box"
        rows = np.nonzero(reach)[0]
        if not len(rows):
            continue
        # 4096 samples per ray on [t0, the crossing or the box's end)
        end = np.minimum(np.where(np.isinf(t), t1, t), t1)[rows]
        ts = t0[rows, None] + (end - t0[rows])[:, None] * (np.arange(4096) / 4096.0)[None]
        depth = np.concatenate([_signed_depth(part, o64[r] + ts[k][:, None] * d64[r]).reshape(1, -1) for k, r in enumerate(rows)])
        start = _signed_depth(part, o64[rows])
        wrong = np.where(start[:, None] > 0, -depth, depth).max(axis=1)   # how far the samples stray to the other side
        # grazing: over its whole stretch in the box the ray gets no deeper into the part, or no nearer to it, than the bound — or it
        # starts within the bound of the boundary
        whole = t0[rows, None] + (t1 - t0)[rows, None] * (np.arange(4096) / 4096.0)[None]
        deepest = np.array([_signed_depth(part, o64[r] + whole[k][:, None] * d64[r]).max() for k, r in enumerate(rows)])
        graze = (np.abs(deepest) <= bound) | (np.abs(start) <= bound)
        hit = ~np.isinf(t[rows])
        at = o64[rows[hit]] + t[rows[hit], None] * d64[rows[hit]]
        off = np.abs(_signed_depth(part, at))
        pairs, grazing, hits = pairs + len(rows), grazing + int(graze.sum()), hits + int(hit.sum())
        if (hit & ~graze).any():
            worst_hit = max(worst_hit, off[~graze[hit]].max())
        worst_side = max(worst_side, wrong[~graze].max())
    print(name, "bound", bound, "pairs", pairs, "hits", hits, "grazing", grazing, "worst hit", worst_hit, "worst stray", worst_side)
    assert hits > 300
    assert grazing <= 0.01 * len(o)
    assert worst_hit <= bound and worst_side <= bound
