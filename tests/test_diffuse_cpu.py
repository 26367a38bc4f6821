"""The reading of the diffuse potentials (tests/diffuse_reading.py) by itself, without a GPU: hand-computed cases, the parameter
mirror, and the conditions tests/test_diffuse_gpu.py relies on, on the committed inputs - every potential is non-zero on a good share
of the standard cloud, no pair sits on the border of a neighbourhood, and the rows whose bound a discontinuous decision widens are at
most 1 % of each cloud.  Prints the distance between the reading in f32 and in f64 beside the derived tolerances."""
import ctypes as C

import numpy as np
import pytest

import diffuse_child as dc
import diffuse_reading as dr
import field_reading as fr

H = float(fr.H32)
VOL = np.float32(1.25e-4)
RHO = 1000.0


@pytest.fixture(scope="module")
def standard():
    case = dr.standard_cloud()
    ref = dr.potentials(case["x"], case["v"], case["vol"], case["rho0"], case["h"])
    return case, ref, dr.crest(case["x"], case["v"], case["h"], ref["normal"])


@pytest.fixture(scope="module")
def shapes():
    case = dr.shapes_cloud()
    ref = dr.potentials(case["x"], case["v"], case["vol"], case["rho0"], case["h"])
    return case, ref, dr.crest(case["x"], case["v"], case["h"], ref["normal"])


def test_two_particles_by_hand():
    d = 0.4 * H
    x = [[0.0, 0.0, 0.0], [d, 0.0, 0.0]]
    wd = 1.0 - d / H
    # approaching head-on: cosine -1, |v_ij| = 2 -> 2 (1 + 1) W_d; separating: cosine +1 -> 0; sliding past: cosine 0, |v_ij| = 1 -> W_d
    for v, expect in (([[1.0, 0, 0], [-1.0, 0, 0]], 4.0 * wd), ([[-1.0, 0, 0], [1.0, 0, 0]], 0.0), ([[0.0, 0, 0], [0.0, 1.0, 0]], wd)):
        got = dr.potentials(x, v, VOL, RHO, H)
        assert got["count"].tolist() == [1, 1]
        assert np.abs(got["trapped_air"] - expect).max() <= 1.0e-12
    # the normals point away from the other particle; both move outwards along them: kappa = (1 - (-1)) W_d
    v = [[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]]
    got = dr.potentials(x, v, VOL, RHO, H, dr.Params(surface_min=0.0))
    assert np.abs(got["normal"] - [[-1.0, 0, 0], [1.0, 0, 0]]).max() <= 1.0e-12
    k = dr.crest(x, v, H, got["normal"])
    assert np.abs(k["wave_crest"] - 2.0 * wd).max() <= 1.0e-12 and k["n"].tolist() == [1, 1]
    # moving inwards: the gate closes
    assert (dr.crest(x, [[1.0, 0, 0], [-1.0, 0, 0]], H, got["normal"])["wave_crest"] == 0).all()
    # energy = m v^2 / 2 with m = V density0 as one f32 product
    m = float(np.float32(VOL) * np.float32(RHO))
    assert np.abs(got["energy"] - 0.5 * m).max() <= 1.0e-15
    # |g| of a pair: V |dW/dr| at d; a threshold above it leaves no normal
    gn = float(VOL) * abs(float(fr.dW(fr.CUBIC, d, H)))
    assert abs(got["gnorm"][0] - gn) <= 1.0e-9 * gn
    assert (dr.potentials(x, v, VOL, RHO, H, dr.Params(surface_min=1.01 * H * gn))["normal"] == 0).all()


def test_three_particles_by_hand():
    d = 0.3 * H
    x = [[-d, 0.0, 0.0], [0.0, 0.0, 0.0], [d, 0.0, 0.0]]
    v = [[0.0, 1.0, 0.0], [0.0, 0.0, 0.0], [0.0, -1.0, 0.0]]
    got = dr.potentials(x, v, VOL, RHO, H, dr.Params(surface_min=0.0))
    assert got["count"].tolist() == [2, 2, 2]
    w1, w2 = 1.0 - d / H, 1.0 - 2.0 * d / H
    # every relative velocity is normal to the line: cosine 0; the ends see |v_ij| = 1 and 2, the middle 1 and 1
    assert np.abs(got["trapped_air"] - [w1 + 2.0 * w2, 2.0 * w1, w1 + 2.0 * w2]).max() <= 1.0e-12
    # the middle's gradient cancels exactly: no normal; the ends point outwards
    assert (got["normal"][1] == 0).all() and got["normal"][0][0] == -1.0 and got["normal"][2][0] == 1.0
    # a particle at the same place is a neighbour, and adds nothing to either sum
    same = dr.potentials([[0.0, 0, 0], [0.0, 0, 0]], [[0.0, 1.0, 0], [1.0, 0, 0]], VOL, RHO, H)
    assert same["count"].tolist() == [1, 1] and (same["trapped_air"] == 0).all() and (same["normal"] == 0).all()
    # a particle that is not finite is nobody's neighbour
    nan = dr.potentials([[np.nan, 0, 0], [0.0, 0, 0]], [[0.0, 1.0, 0], [1.0, 0, 0]], VOL, RHO, H)
    assert nan["count"].tolist() == [0, 0] and (nan["energy"][0] == 0)


def test_the_python_defaults_are_the_librarys(hip_lib):
    from salva_amd import Diffuse, _lib

    assert C.sizeof(_lib.DiffuseParams) == _lib.DIFFUSE_BYTES == 128 and C.sizeof(_lib.DiffuseStats) == _lib.DIFFUSE_STATS_BYTES == 104
    p = _lib.DiffuseParams()
    hip_lib.salva_hip_default_diffuse(C.byref(p))
    assert bytes(p) == bytes(Diffuse()._struct())
    assert (p.surface_min, p.crest_cos) == (dr.Params().surface_min, np.float32(dr.Params().crest_cos))
    assert bytes(p) == bytes(dc.mirror(dr.Params())._struct())  # the reading's defaults too
    assert (p.n_spray, p.n_bubble, p.has_kill_box, p.max_per_particle) == (6, 20, 0, 16) and list(p.gravity) == [0.0, np.float32(-9.81), 0.0]
    box = Diffuse(kill_box=((0, 1, 2), (3, 4, 5)))._struct()
    assert box.has_kill_box == 1 and list(box.kill_lo) == [0, 1, 2] and list(box.kill_hi) == [3, 4, 5]


@pytest.mark.parametrize("which", ["standard", "shapes"])
def test_the_inputs_meet_their_conditions(which, request):
    case, ref, k = request.getfixturevalue(which)
    n = len(case["x"])
    assert len(dr.near_the_border(case["x"], case["h"])) == 0
    _, wide_n = dr.normal_bounds(ref)
    wide = wide_n | (k["at_stake"] > 0) | k["close"]
    print(f"{which}: {n} rows, {int(wide.sum())} with a widened bound ({int(wide_n.sum())} normal, {int((k['at_stake'] > 0).sum())} sign, "
          f"{int(k['close'].sum())} gate)")
    assert wide.sum() <= 0.01 * n
    # f32 against f64: what the arithmetic itself costs, beside what the tolerances allow
    r32 = dr.potentials(case["x"], case["v"], case["vol"], case["rho0"], case["h"], dtype=np.float32)
    assert np.array_equal(r32["count"], ref["count"])
    tol = dr.tol_sum(ref["n"], ref["A_trapped"], dr.C_TRAPPED)
    err = np.abs(r32["trapped_air"].astype(np.float64) - ref["trapped_air"])
    print(f"trapped_air: f32 - f64 at most {float((err[tol > 0] / tol[tol > 0]).max()):.4f} of the tolerance")
    assert (err <= tol).all()
    tol_n, _ = dr.normal_bounds(ref)
    both = ref["has_normal"] & r32["has_normal"]
    err = np.sqrt(((r32["normal"].astype(np.float64) - ref["normal"]) ** 2).sum(axis=1))
    print(f"normal: f32 - f64 at most {float((err[both] / tol_n[both]).max()):.4f} of the tolerance over {int(both.sum())} rows")
    assert (err[both] <= tol_n[both]).all()
    k32 = dr.crest(case["x"], case["v"], case["h"], ref["normal"].astype(np.float32), dtype=np.float32)
    k64 = dr.crest(case["x"], case["v"], case["h"], ref["normal"].astype(np.float32))
    dr.compare_crest(k32["wave_crest"], k64)


def test_the_standard_cloud_exercises_every_potential(standard):
    case, ref, k = standard
    n = len(case["x"])
    share = {"trapped_air": (ref["trapped_air"] > 0).mean(), "normal": ref["has_normal"].mean(), "wave_crest": (k["wave_crest"] > 0).mean(),
             "energy": (ref["energy"] > 0).mean()}
    print({a: round(float(b), 3) for a, b in share.items()}, "neighbours", int(ref["count"].min()), "to", int(ref["count"].max()))
    assert share["trapped_air"] > 0.9 and share["energy"] > 0.9 and 0.2 < share["normal"] < 0.8 and share["wave_crest"] > 0.1
    assert (k["wave_crest"][ref["has_normal"]] == 0).any()  # the gate closes somewhere
    assert n == 1386 and case["n0"] not in (0, n)  # two fluids


def test_the_shapes_are_what_they_are_named(shapes):
    case, ref, k = shapes
    parts = case["parts"]
    assert ref["count"][parts["lone"]].tolist() == [0] and ref["count"][parts["stray"]].tolist() == [0]
    assert ref["count"][parts["pair"]].tolist() == [1, 1] and ref["count"][parts["same"]].tolist() == [1, 1]
    assert ref["count"][parts["nan"]].tolist() == [0] and (ref["energy"][parts["nan"]] == 0).all()
    assert (ref["trapped_air"][parts["same"]] == 0).all() and (ref["normal"][parts["same"]] == 0).all()
    # eps < r <= 1e-5 h: the cubic spline's gradient is zero (the pair has no normal even at surface_min = 0), W_d is not
    close = case["x"][parts["close"]].astype(np.float64)
    assert fr.EPS < np.linalg.norm(close[0] - close[1]) <= 1.0e-5 * case["h"]
    assert ref["count"][parts["close"]].tolist() == [1, 1] and (ref["gnorm"][parts["close"]] == 0).all() and (ref["trapped_air"][parts["close"]] > 0).all()
    assert ref["count"][parts["line"]].max() <= 4 and ref["count"][parts["sheet"]].max() <= 14
    rest = case["rest"]
    assert ref["energy"][rest] == 0 and ref["trapped_air"][rest] > 0 and k["wave_crest"][rest] == 0 and ref["count"][rest] > 20
    assert not ref["has_normal"][rest]  # deep inside
    assert ref["has_normal"][parts["block"]].any() and (k["wave_crest"][parts["block"]] > 0).any()


def test_phi_at_and_beyond_its_ends():
    lo, hi = 5.0, 20.0
    assert [float(dr.phi(v, lo, hi)) for v in (-1.0, 0.0, 5.0, 20.0, 21.0, np.inf)] == [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
    assert float(dr.phi(12.5, lo, hi)) == 0.5
    p = dr.phi(np.linspace(0.0, 30.0, 301), lo, hi)
    assert p.dtype == np.float32 and (np.diff(p) >= 0).all() and p.min() == 0.0 and p.max() == 1.0


def test_the_mixing_function_has_the_headers_values():
    """the values written down in include/salva_hip.h, read from it"""
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "salva_hip.h")).read()
    text = re.sub(r"\n \*\s+", " ", text)
    m = re.search(r"fmix\(0\) = 0, fmix\(1\) = (0x[0-9a-f]{8}) and bits\(0\) for seed = updates = slot = index = 0 is 0; for seed 1, updates 2, slot 3, "
                  r"index 4: bits\(5\) = (0x[0-9a-f]{8})", text)
    assert m, "the header's values"
    assert dr.fmix(0) == 0 and dr.fmix(1) == int(m.group(1), 16) and dr.bits(0, 0, 0, 0, 0) == 0 and dr.bits(1, 2, 3, 4, 5) == int(m.group(2), 16)
    assert "0x7feb352d" in text and "0x846ca68b" in text
    # on arrays as on integers; a uniform is a multiple of 2^-24 in [0, 1)
    idx = np.arange(1000, dtype=np.uint64)
    k = dr.key(7, 3, 1, idx)
    assert all(int(k[i]) == dr.key(7, 3, 1, int(i)) for i in (0, 1, 999))
    u = np.array([dr.uniform(int(kk), 0) for kk in k[:200]])
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all() and ((u * 2.0 ** 24) % 1 == 0).all() and 0.4 < u.mean() < 0.6
    assert len(np.unique(k)) == 1000


def test_the_disc_rejection_stays_inside_the_disc():
    pts = np.array([dr.disc(dr.key(5, 0, 0, i), 1 + 20 * j) for i in range(300) for j in range(3)], np.float64)
    r2 = (pts ** 2).sum(axis=1)
    assert (r2 <= 1.0).all() and r2.max() > 0.9 and (pts.min(axis=0) < -0.8).all() and (pts.max(axis=0) > 0.8).all()
    assert 0.4 < r2.mean() < 0.6  # uniform on the disc: E r^2 = 1/2
    # the frame is orthonormal to the direction of motion, whichever axis is the smallest
    for v in ([1.0, 2.0, 3.0], [3.0, -1.0, 2.0], [2.0, 3.0, 0.0], [0.0, 0.0, -2.0], [1.0, 1.0, 1.0]):
        v = np.float32(v)
        e1, e2 = dr.frame(v)
        w = v.astype(np.float64) / np.linalg.norm(v)
        gram = np.array([[a @ b for b in (w, e1.astype(np.float64), e2.astype(np.float64))] for a in (w, e1.astype(np.float64), e2.astype(np.float64))])
        assert np.abs(gram - np.eye(3)).max() <= 8.0 * dr.U


def test_the_emission_parameters_do_what_the_gpu_test_needs(standard):
    case, ref, k = standard
    slot, index = dc.standard_rows(case)
    pot = {"trapped_air": ref["trapped_air"].astype(np.float32), "wave_crest": k["wave_crest"].astype(np.float32), "energy": ref["energy"].astype(np.float32)}
    p = dc.emit_params()
    new, (emitted, dropped), c = dr.emit(case["x"], case["v"], slot, index, pot, p, dc.EMIT_DT, 0, case["r"], 0, 10 ** 6)
    print(f"{emitted} emitted by {int((c > 0).sum())} rows, {int((c == p.max_per_particle).sum())} at the limit, {int((c == 0).sum())} rows emit nothing")
    assert 200 <= emitted <= 2000 and dropped == 0 and (c == p.max_per_particle).sum() >= 5 and (c == 0).sum() >= 100
    # a new particle lies within r of its parent's path over the step
    parent = np.repeat(np.arange(len(c)), c)
    d = new["positions"].astype(np.float64) - case["x"][parent]
    assert (np.linalg.norm(d, axis=1) <= case["r"] + dc.EMIT_DT * np.linalg.norm(case["v"][parent], axis=1) + 1e-6).all()
    assert (new["lifetime"] >= 2.0).all() and (new["lifetime"] <= 5.0).all() and np.array_equal(new["id"], np.arange(emitted))
    # advection by hand: spray falls, foam follows and ages, a bubble rises against gravity and is dragged
    q = dr.Params()
    one = lambda n: dr.advect([[0.0, 0, 0]], [[1.0, 0, 0]], [3.0], [9], [n], [[0.0, 2.0, 0]], q, 0.5)[0]  # noqa: E731
    assert np.allclose(one(0)["velocities"], [[1.0, -4.905, 0]]) and one(0)["kind"][0] == dr.SPRAY and one(0)["lifetime"][0] == 3.0
    assert np.array_equal(one(6)["velocities"], np.float32([[0.0, 2.0, 0]])) and one(6)["kind"][0] == dr.FOAM and one(6)["lifetime"][0] == 2.5
    assert one(20)["kind"][0] == dr.FOAM and one(21)["kind"][0] == dr.BUBBLE
    assert np.allclose(one(21)["velocities"], [[1.0 - 0.8, 9.81 + 0.8 * 2.0, 0]]) and np.allclose(one(6)["positions"], [[0.0, 1.0, 0]])
    gone, (dissolved, killed) = dr.advect([[0.0, 0, 0], [np.nan, 0, 0]], np.zeros((2, 3)), [0.25, 3.0], [4, 5], [10, 10], np.zeros((2, 3)), q, 0.5)
    assert len(gone["id"]) == 0 and (dissolved, killed) == (1, 1)
