"""Ray casts at the fluid without a GPU: the library exports the entry points, the f32 reading of the contract
(tests/fluid_ray_reading.py) means what an f64 geometric ray / sphere intersection means, the camera formula, and the walk's margin
eps covers the standard case.

Only the first test touches the library.  The other three exercise numpy code under tests/ alone and would pass without the feature:
they show that the reading, which the GPU tests hold the device to, is sound.  `walk_covers` and `cast_eps` of the reading are a hand
copy of the walk in salva_amd/csrc/fluidcast.hip; nothing ties the copy's constants (1.75, 2^-19) to the kernel's but the GPU tests'
bit-for-bit comparison, which fails if the kernel's walk leaves out a cell."""
import numpy as np
import pytest

import fluid_ray_reading as rr

F = np.float32


@pytest.fixture(scope="module")
def case():
    return rr.standard_case()


@pytest.fixture(scope="module")
def reading(case):
    return rr.cast(case["origins"], case["directions"], case["x"], case["slots"], case["radii"][0])


def test_the_library_exports_the_entry_points(hip_lib):
    from salva_amd import _lib

    for name in ("salva_hip_cast_rays", "salva_hip_cast_rays_camera"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    import ctypes as C

    assert C.sizeof(_lib.RayParams) == _lib.RAY_PARAMS_BYTES and C.sizeof(_lib.RayCamera) == _lib.RAY_CAMERA_BYTES
    assert C.sizeof(_lib.RayOut) == 5 * C.sizeof(C.c_void_p)


def test_the_reading_against_f64_geometry(case, reading):
    """The bound on t, as a length (t |d|).  With M = the largest coordinate in play (origins included) one f32 rounding of a
    position is at most u = 2^-24 M.  An error of ta alone does not matter: o' = o + ta d stays on the ray, and t = ta + (the cast
    from o') gives the shift back.  What matters is e = 8 u: the rounding of o' (two operations per component, 2 sqrt(3) u < 3.5 u as
    a vector), of q (1 u) and ray_ball's own (p: 3 u; the dots: < 0.5 u).  A displacement e of the line changes the entry point of a
    sphere met at distance p from its centre by at most e (1 + p / sqrt(R^2 - p^2)); for a sphere not grazed within g, R - p >= g,
    that is at most e (1 + sqrt(R / g)) since R^2 - p^2 >= R g.  The final sum ta + t rounds once more: 2^-24 T, T the longest
    t |d|.  Choosing g = tau gives tau = e (1 + sqrt(R / tau)) + 2^-24 T, solved below by iteration (about 4e-5 here, R / 600).
    Left out of the identity comparison: rays where a sphere grazed within tau in f64 (|p - R| < tau: met or not, its f32 entry may
    move by up to sqrt(2 R tau) + tau) could be the winner - its closest approach tm lies no later than the best t plus that - rays
    whose two best f64 candidates lie within 2 tau of each other, and rays that start within tau of a sphere's surface (t1 ~ 0: the
    candidate's existence may flip).  Everywhere else the winner is the same particle and |t32 - t64| |d| <= tau."""
    o, d, x, R = case["origins"], case["directions"], case["x"], case["radii"][0]
    M = max(np.abs(o).max(), np.abs(x).max())
    dn = np.linalg.norm(d.astype(np.float64), axis=1)
    tm, p, t0, t1 = rr.cast_f64(o, d, x, R)
    u = 2.0 ** -24 * M
    e = 8 * u
    with np.errstate(invalid="ignore"):
        tj = np.where((t1 >= 0), np.maximum(t0, 0.0), np.inf)  # NaN (not met) compares false
    T = (np.where(np.isfinite(tj), tj, 0.0).max(axis=1) * dn).max()
    tau = e
    for _ in range(50):
        tau = e * (1 + np.sqrt(R / tau)) + 2.0 ** -24 * T
    print("tau =", tau, "= R /", R / tau)
    order = np.sort(tj, axis=1)
    best, second = order[:, 0], order[:, 1]
    win = tj.argmin(axis=1)
    hit64 = np.isfinite(best)
    slack = (np.sqrt(2 * R * tau) + tau)
    grazed = np.abs(p - R) < tau
    with np.errstate(invalid="ignore"):
        risky = grazed & (tm * dn[:, None] >= -slack) & ((tm * dn[:, None]) <= (np.where(hit64, best, np.inf) * dn + slack)[:, None])
        close = hit64 & ((second - best) * dn < 2 * tau)
        onsurface = (np.abs(np.nan_to_num(t1, nan=np.inf)) * dn[:, None] < tau).any(axis=1)
    left_out = risky.any(axis=1) | close | onsurface
    print("left out:", int(left_out.sum()), "of", len(o), "(grazes", int(risky.any(axis=1).sum()), ", close pairs", int(close.sum()), ", on a surface",
          int(onsurface.sum()), ")")
    assert left_out.mean() <= 0.02
    keep = ~left_out
    hit32 = reading["row"] >= 0
    assert np.array_equal(hit32[keep], hit64[keep])
    both = keep & hit64
    assert both.sum() > 1000 and (keep & ~hit64).sum() > 10  # hits and misses both occur
    assert np.array_equal(reading["row"][both], win[both])
    err = np.abs(reading["t"][both].astype(np.float64) - best[both]) * dn[both]
    print("max |t32 - t64| |d| =", err.max())
    assert err.max() <= tau
    # the normal is the unit vector from the centre to the hit point
    hitp = o[both].astype(np.float64) + best[both][:, None] * d[both]
    n64 = (hitp - x[win[both]]) / R
    inside = best[both] == 0.0  # (a ray that starts inside its sphere: the normal points from the centre to o)
    assert np.abs(reading["normal"][both][~inside] - n64[~inside]).max() < 64 * tau / R
    # and the thickness is the summed chord length
    with np.errstate(invalid="ignore"):
        chord = np.nan_to_num(np.maximum(t1, 0.0) - np.maximum(t0, 0.0), nan=0.0).clip(min=0.0).sum(axis=1)
    calm = ~grazed.any(axis=1)
    assert (np.abs(reading["thickness"][calm] - chord[calm]) * dn[calm] <= (reading["n"][calm] + 1) * 2 * tau).all()


def test_the_camera_formula_by_hand():
    cam = {"origin": [1.0, 2.0, 3.0], "forward": [0.0, 0.0, -1.0], "right": [0.5, 0.0, 0.0], "up": [0.0, 0.25, 0.0], "width": 3, "height": 2}
    o, d = rr.camera_rays(cam)
    assert o.shape == d.shape == (6, 3) and (o == np.array([1.0, 2.0, 3.0], F)).all()
    # su = (ix + 0.5) * (2 / 3) - 1 in f32, sv = (iy + 0.5) * 1 - 1 = -0.5, +0.5
    third = F(2.0) / F(3.0)
    su = [F(F(F(0.5) * third) - F(1.0)), F(F(F(1.5) * third) - F(1.0)), F(F(F(2.5) * third) - F(1.0))]
    assert su[1] == 0.0 and abs(float(su[0]) + 2.0 / 3.0) < 1e-7 and abs(float(su[2]) - 2.0 / 3.0) < 1e-7
    for iy, sv in enumerate((F(-0.5), F(0.5))):
        for ix in range(3):
            want = np.array([F(su[ix] * F(0.5)), F(sv * F(0.25)), F(-1.0)], F)
            assert np.array_equal(d[iy * 3 + ix], want), (ix, iy)


def test_eps_covers_the_standard_case(case):
    """Every (ray, particle) pair that the f32 cast meets lies in a cell the dilated walk visits - for both radii of the GPU test, and
    for the same block 1 000 h away from the origin, where one rounding is sixty times larger."""
    for R in case["radii"]:
        met, missed = rr.walk_covers(case["origins"], case["directions"], case["x"], R, case["h"])
        print("R =", R, ":", met, "pairs met,", missed, "outside the walk")
        assert met > 10000 and missed == 0
    shift = np.array([100.0, -100.0, 50.0], F)
    sub = slice(0, 1024)
    met, missed = rr.walk_covers(case["origins"][sub] + shift, case["directions"][sub], case["x"] + shift, case["radii"][1], case["h"])
    print("shifted:", met, "pairs met,", missed, "outside the walk")
    assert met > 2000 and missed == 0
