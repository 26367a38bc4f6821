"""A brute-force reading of the field evaluator's semantics (include/salva_hip.h salva_hip_evaluate_fields): plain
numpy, float64, all pairs, no grid.  Written from the header's contract and from the reference's kernel formulas (kernel/
cubic_spline_kernel.rs, poly6_kernel.rs, spiky_kernel.rs, viscosity_kernel.rs, kernel.rs:13-24), not from the device code, and it shares
no code with tests/numpy_reading.py (tests/test_field_cpu.py compares the two).

For every point and every sum S = sum_j a_j K_j it returns S, the number n of particles in support and A = sum_j |a_j| K_max, where
K_max is the largest magnitude of W (resp. |dW/dr|) on [q_min, 1] and q_min the smallest pair distance of the whole case over h, both
taken numerically.

The tolerance is derived, not chosen.  A device value may differ from the reading by at most (n + 16) 2^-24 A: n - 1 roundings of an
f32 sum in any order, and 16 for the dozen roundings of one term (three differences, r^2, the reciprocal root at 1 ulp, q, the
polynomial).  A is in units of K_max and not of the term, because the cancellation in (1 - q)^3 near q = 1 is absolute, not relative.
For velocity = P / rho the bound is first-order propagation: (tol_P + |v_ref| tol_rho) / rho_ref + 2 2^-24 |v_ref|.  Counts and exact
zeros (empty support, non-finite points) are compared exactly.

Test infrastructure only."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
CUBIC, POLY6, SPIKY, VISCOSITY = 0, 1, 2, 3
EPS = float(np.finfo(np.float32).eps)  # kernel.rs:19: the gradient is zero when |d| <= eps


def W(kind, r, h):
    """W(r) for r in [0, h] (the caller masks the support)."""
    q = r / h
    if kind == CUBIC:  # cubic_spline_kernel.rs:12-33, dim 3: 8 / (pi h^3) * (1 - 6 q^2 + 6 q^3 | 2 (1 - q)^3)
        return 8.0 / (np.pi * h ** 3) * np.where(q <= 0.5, 1.0 + 6.0 * (q ** 3 - q ** 2), 2.0 * (1.0 - q) ** 3)
    if kind == POLY6:  # poly6_kernel.rs: 315 / (64 pi h^9) (h^2 - r^2)^3
        return 315.0 / (64.0 * np.pi * h ** 9) * (h * h - r * r) ** 3
    if kind == SPIKY:  # spiky_kernel.rs: 15 / (pi h^6) (h - r)^3
        return 15.0 / (np.pi * h ** 6) * (h - r) ** 3
    # viscosity_kernel.rs: 15 / (2 pi h^3) (r^2 / h^2 (1 - r / 2h) + h / 2r - 1) for r > 0, 0 at r = 0
    s = np.where(r > 0.0, r, 1.0)
    return np.where(r > 0.0, 15.0 / (2.0 * np.pi * h ** 3) * (s * s / (h * h) * (1.0 - s / (2.0 * h)) + h / (2.0 * s) - 1.0), 0.0)


def dW(kind, r, h):
    """dW/dr for r in [0, h]."""
    q = r / h
    if kind == CUBIC:  # cubic_spline_kernel.rs:55-79: zero for q <= 1e-5
        inner, outer = 6.0 * q * (3.0 * q - 2.0), -6.0 * (1.0 - q) ** 2
        return 8.0 / (np.pi * h ** 4) * np.where(q <= 1.0e-5, 0.0, np.where(q <= 0.5, inner, outer))
    if kind == POLY6:
        return 315.0 / (64.0 * np.pi * h ** 9) * -6.0 * r * (h * h - r * r) ** 2
    if kind == SPIKY:
        return -45.0 / (np.pi * h ** 6) * (h - r) ** 2
    s = np.where(r > 0.0, r, 1.0)
    return np.where(r > 0.0, 15.0 / (2.0 * np.pi * h ** 3) * (-3.0 * s * s / (2.0 * h ** 3) + 2.0 * s / (h * h) - h / (2.0 * s * s)), 0.0)


def k_max(fn, kind, h, q_min):
    q = np.unique(np.concatenate([np.linspace(min(q_min, 1.0), 1.0, 20001), [min(q_min, 1.0), 0.5, 1.0]]))
    return float(np.abs(fn(kind, q * h, h)).max())


def find_pairs(points, x, h, border=0.0, chunk=2048):
    """Every (point, particle) pair with r^2 <= h^2, by testing all of them: a dict of the pairs' point and particle indices, their
    d = x - x_j and r, and per point whether one of its pairs lies within `border` of distance h; `r_min`: the smallest distance of all
    pairs, in support or not."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    x, h = np.asarray(x, np.float64).reshape(-1, 3), float(h)
    finite = np.isfinite(pts).all(axis=1)
    pi, pj, pd, pr, near, r_min = [], [], [], [], np.zeros(len(pts), bool), np.inf
    for a in range(0, len(pts), chunk):
        f = finite[a:a + chunk]
        p = np.where(f[:, None], pts[a:a + chunk], 0.0)
        d = p[:, None, :] - x[None, :, :]
        r = np.sqrt((d * d).sum(axis=2))
        s = (r * r <= h * h) & f[:, None]
        i, j = np.nonzero(s)
        pi.append(i + a); pj.append(j); pd.append(d[i, j]); pr.append(r[i, j])
        near[a:a + chunk] = ((np.abs(r - h) <= border) & f[:, None]).any(axis=1)
        if f.any() and len(x):
            r_min = min(r_min, float(r[f].min()))
    return {"m": len(pts), "i": np.concatenate(pi), "j": np.concatenate(pj), "d": np.concatenate(pd), "r": np.concatenate(pr), "border": near,
            "r_min": r_min, "h": h}


def evaluate(points, x, v, vol, rho0, h, kd=CUBIC, kg=CUBIC, q_min=None, border=0.0, pairs=None):
    """points: (m, 3); x, v: (n, 3); vol, rho0: (n) - rho0 the rest density of each particle's fluid; h: the kernel radius.  `pairs`: the
    result of find_pairs for the same points, particles and h (it does not depend on the kernels).  Returns a dict of float64 arrays."""
    if pairs is None:
        pairs = find_pairs(points, x, h, border)
    v = np.asarray(v, np.float64).reshape(-1, 3)
    vol, rho0, h = np.asarray(vol, np.float64), np.asarray(rho0, np.float64), float(h)
    mass = vol * rho0
    m, i, j, d, r = pairs["m"], pairs["i"], pairs["j"], pairs["d"], pairs["r"]
    if q_min is None:
        q_min = pairs["r_min"] / h
    kw, kg_max = k_max(W, kd, h, q_min), k_max(dW, kg, h, q_min)

    def total(values):
        return np.bincount(i, weights=values, minlength=m)

    w = W(kd, r, h)
    g = np.where(r > EPS, dW(kg, r, h), 0.0)
    direction = d / np.where(r > 0.0, r, 1.0)[:, None]
    out = {"n": np.bincount(i, minlength=m).astype(np.int64), "density": total(w * mass[j]), "fraction": total(w * vol[j]),
           "P": np.stack([total(w * mass[j] * v[j, a]) for a in range(3)], axis=1),
           "gradient": np.stack([total(g * mass[j] * direction[:, a]) for a in range(3)], axis=1),
           "A_density": total(mass[j]) * kw, "A_fraction": total(vol[j]) * kw,
           "A_P": np.stack([total(np.abs(mass[j] * v[j, a])) for a in range(3)], axis=1) * kw, "A_gradient": total(mass[j]) * kg_max,
           "border": pairs["border"], "q_min": q_min}
    rho = out["density"]
    out["velocity"] = np.where((rho != 0.0)[:, None], out["P"] / np.where(rho != 0.0, rho, 1.0)[:, None], 0.0)
    return out


def tol_sum(n, A):
    """what a device sum may differ by"""
    return (np.asarray(n, np.float64) + 16.0) * U * np.asarray(A, np.float64)


def tol_velocity(ref):
    """per component, where the reference density is not zero"""
    rho = np.where(ref["density"] != 0.0, ref["density"], 1.0)[:, None]
    tp, tr = tol_sum(ref["n"][:, None], ref["A_P"]), tol_sum(ref["n"], ref["A_density"])[:, None]
    return (tp + np.abs(ref["velocity"]) * tr) / rho + 2.0 * U * np.abs(ref["velocity"])


def compare(got, ref, skip_border_count=True, fields=("density", "fraction", "velocity", "gradient", "count")):
    """Asserts every field of `got` (the evaluator's dict, flat arrays) against the reading at the derived tolerance; prints the worst
    ratio error / tolerance of each float field first."""
    m = len(ref["n"])
    empty = ref["n"] == 0
    for name in fields:
        if name not in got:
            continue
        g = np.asarray(got[name])
        if name == "count":
            keep = ~ref["border"] if skip_border_count else np.ones(m, bool)
            bad = np.nonzero((g.reshape(m).astype(np.int64) != ref["n"]) & keep)[0]
            assert len(bad) == 0, (name, bad[:5], g.reshape(m)[bad[:5]], ref["n"][bad[:5]])
            continue
        g = g.astype(np.float64).reshape(m, -1)
        r = np.asarray(ref[name], np.float64).reshape(m, -1)
        if name == "velocity":
            tol = tol_velocity(ref)
        elif name == "gradient":
            tol = np.repeat(tol_sum(ref["n"], ref["A_gradient"])[:, None], 3, axis=1)
        else:
            tol = tol_sum(ref["n"], ref["A_" + name])[:, None]
        assert np.isfinite(g).all(), name
        assert (g[empty] == 0.0).all(), (name, "not exactly zero where the support is empty")
        err = np.abs(g - r)
        some = ~empty[:, None] & (tol > 0.0)
        ratio = float((err[some] / tol[some]).max()) if some.any() else 0.0
        print(f"{name}: worst error / tolerance = {ratio:.3f} over {int((~empty).sum())} places")
        worst = np.unravel_index(np.argmax(err - tol), err.shape)
        assert (err <= tol).all(), (name, worst, g[worst], r[worst], tol[worst], int(ref["n"][worst[0]]))


# ------------------------------------------------------------------------------------------------ the standard case
R = 0.025
SMOOTHING = 2.0
H32 = F32(F32(R) * F32(SMOOTHING) * F32(2.0))  # liquid_world.rs:44 in f32, as the library computes it
GRID = (14, 11, 9)
DENSITY0 = (1000.0, 500.0)


def standard_case(seed=7):
    """r = 0.025, h = 4 r; a 14 x 11 x 9 lattice at 2 r jittered by +-0.2 r, split into two fluids by x (density0 1000 and 500, fluid 0
    first: host order), volumes 0.8 (2r)^3 (1 + 0.25 i / n), velocities distinct per particle and component; 3 001 points uniform in
    the particles' (nominal) box grown by 1.5 h; a lattice over the same box at spacing r: 39 x 33 x 29 nodes."""
    rng = np.random.default_rng(seed)
    r, h = R, float(H32)
    ix, iy, iz = np.meshgrid(np.arange(GRID[0]), np.arange(GRID[1]), np.arange(GRID[2]), indexing="ij")
    cell = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1)
    x = cell * (2.0 * r) + rng.uniform(-0.2 * r, 0.2 * r, (len(cell), 3))
    first = cell[:, 0] < GRID[0] // 2
    order = np.concatenate([np.nonzero(first)[0], np.nonzero(~first)[0]])
    x = x[order].astype(F32)
    n, n0 = len(x), int(first.sum())
    i = np.arange(n)
    vol = (0.8 * (2.0 * r) ** 3 * (1.0 + 0.25 * i / n)).astype(F32)
    v = np.stack([np.sin(0.37 * i) + 0.1, 0.5 * np.cos(0.11 * i) - 0.2, 0.3 * np.sin(0.7 * i + 1.0) + 0.05 * i / n], axis=1).astype(F32)
    rho0 = np.where(i < n0, DENSITY0[0], DENSITY0[1]).astype(np.float64)
    lo = np.zeros(3) - 1.5 * h
    hi = (np.array(GRID) - 1) * 2.0 * r + 1.5 * h
    points = rng.uniform(lo, hi, (3001, 3)).astype(F32)
    origin = lo.astype(F32)
    spacing = F32(r)
    dims = tuple(int(round((hi[a] - lo[a]) / r)) + 1 for a in range(3))
    return {"r": r, "h": h, "x": x, "v": v, "vol": vol, "rho0": rho0, "n0": n0, "points": points, "origin": origin, "spacing": spacing,
            "dims": dims, "nodes": lattice_nodes(origin, spacing, dims)}


def lattice_nodes(origin, spacing, dims):
    """node (ix, iy, iz) at origin + (float)i * spacing, product and sum each rounded in f32; row (ix ny + iy) nz + iz"""
    axes = [(np.asarray(origin, F32)[a] + (np.arange(dims[a]).astype(F32) * F32(spacing)).astype(F32)).astype(F32) for a in range(3)]
    gx, gy, gz = np.meshgrid(*axes, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1).astype(F32)
