"""A brute-force reading of the anisotropic kernels (include/salva_hip.h "Anisotropic kernels"): plain numpy, all pairs,
no grid, numpy.linalg.eigh.  Written from the header's contract, not from the device code; the kernel formulas P and P' are those of
tests/field_reading.py evaluated with h = 1.

`moments` runs in float64, or in float32 throughout (dtype=numpy.float32): the distance between the two runs on the same cloud is the
yardstick for salva_hip_compute_anisotropy (tests/test_anisotropy_gpu.py allows 4 x that distance, because the device's Jacobi and its
order of summation are not numpy's).

`evaluate` takes centres and metrics as they are given - the device's own, in the GPU tests, so that only the sums are under test - and
returns, per place and per sum S = sum_j a_j det G_j K(q_j), the value, the number n of particles with q_j <= 1 and
A = sum_j |a_j| det G_j K_max (for the gradient: times |G_j|, the largest eigenvalue), K_max the largest magnitude of P (resp. P') on
[q_min, 1] and q_min the smallest q of the case, both taken numerically.

The tolerance is derived, not chosen: a device value may differ from the reading by at most (n + c) 2^-24 A.  n - 1 roundings of an f32
sum in any order, and c for one term, with u = 2^-24 and kappa = S_HI / S_LO = 8 the largest ratio of two eigenvalues of a metric:
  16      the term's own roundings, as in tests/field_reading.py (q^2, the reciprocal root, q, the polynomial, the products);
  92 L    q through the metric.  d = x - c: u |d|.  y = G d: three products and two sums per component, each bounded by |G_k| |d|,
          and the error of d carried along: 6 u |G|_F |d| <= 6 sqrt(3) u |G| |d| <= 10.4 kappa u q, since |d| <= q / lambda_min(G).
          The sum of squares, the reciprocal root and the product: 4 u q more.  So dq <= (10.4 kappa + 4) u q < 92 u q, and
          |dK| <= max(q |K'(q)|) dq / q: L = max q |K'(q)| / K_max on [q_min, 1], taken numerically (below 1 for all four kernels);
  320     det G.  The device multiplies the three quotients 1 / (h s_k) (11 u); the reading takes the determinant of the six f32
          entries it is given.  Those are sums of three products of f32 factors (8 u |G| each, 24 kappa u = 192 u on the
          determinant), of eigenvectors that fifteen Jacobi rotations, each orthogonal to 4 u in f32, leave orthogonal to 60 u -
          120 u on the determinant of R diag R^T.  11 + 192 + 120 < 320.
For the gradient, a_j det G_j (P'(q) / q) G y, add 92 for the direction y / q (the bound on dy above) and 48 = 6 kappa for the second
product with G: c = 476 + 92 L with L taken from P' and P''.  Exact zeros are required where no particle reaches.

Test infrastructure only."""
from dataclasses import dataclass

import numpy as np

import field_reading as fr

F32 = np.float32
U = fr.U
S_LO, S_HI = 0.25, 2.0  # SALVA_HIP_ANISOTROPY_S_LO / _S_HI
KAPPA = S_HI / S_LO
NEVER_ISOLATED_OFF = 2 ** 32 - 1


@dataclass
class Params:
    """SalvaHipAnisotropy; the defaults are salva_hip_default_anisotropy's"""
    lam: float = 0.9
    k_r: float = 4.0
    k_s: float = 5.0 / 3.0
    k_n: float = 0.5
    n_eps: int = 25


def valid(p):
    """what the header accepts"""
    return bool(0.0 <= p.lam <= 1.0 and np.isfinite(p.k_r) and p.k_r >= 1.0 and np.isfinite(p.k_s) and p.k_s > 0.0 and S_LO <= p.k_n <= S_HI)


def moments(x, h, p=None, dtype=np.float64):
    """x: (n, 3) positions of the selected particles.  Returns a dict: `centres` (n, 3), `metric` (n, 6: xx, xy, xz, yy, yz, zz of G),
    `count` (n), `s` (n, 3: the stretches, descending eigenvalue of C), all computed in `dtype`.  A non-finite row: its position, a zero
    metric, count 0."""
    p = p or Params()
    T = dtype
    x = np.asarray(x, T).reshape(-1, 3)
    n = len(x)
    h = T(h)
    R = T(h + h)
    R2 = T(R * R)
    finite = np.isfinite(x).all(axis=1)
    centres, metric, count, stretch = x.copy(), np.zeros((n, 6), T), np.zeros(n, np.int64), np.zeros((n, 3), T)
    xs = np.where(finite[:, None], x, T(0))
    for i in np.nonzero(finite)[0]:
        d = (xs - xs[i]).astype(T)
        r2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(T)
        near = finite & (r2 <= R2)
        d, r2 = d[near], r2[near]
        t = (np.sqrt(r2) / R).astype(T)
        w = (T(1) - t * t * t).astype(T)
        s0 = w.sum(dtype=T)
        s1 = (w[:, None] * d).sum(axis=0, dtype=T)
        s2 = (w[:, None, None] * d[:, :, None] * d[:, None, :]).sum(axis=0, dtype=T)
        m = (s1 / s0).astype(T)
        c = (s2 / s0 - np.outer(m, m)).astype(T)
        count[i] = near.sum() - 1
        centres[i] = (x[i] + T(p.lam) * m).astype(T)
        if count[i] > p.n_eps:
            sigma, rot = np.linalg.eigh(c)  # ascending
            sigma, rot = sigma[::-1].astype(T), rot[:, ::-1].astype(T)
            s = np.minimum(np.maximum(T(p.k_s) * np.maximum(sigma, sigma[0] / T(p.k_r)) / (h * h), T(S_LO)), T(S_HI)).astype(T)
            g = ((rot * (T(1) / s)[None, :]) @ rot.T / h).astype(T)
        else:
            s = np.full(3, T(p.k_n))
            g = (np.eye(3, dtype=T) / (T(p.k_n) * h)).astype(T)
        stretch[i] = s
        metric[i] = (g[0, 0], g[0, 1], g[0, 2], g[1, 1], g[1, 2], g[2, 2])
    return {"centres": centres, "metric": metric, "count": count, "s": stretch, "finite": finite}


def full(metric):
    """(n, 6) -> (n, 3, 3)"""
    m = np.asarray(metric, np.float64)
    g = np.empty((len(m), 3, 3))
    g[:, 0, 0], g[:, 0, 1], g[:, 0, 2], g[:, 1, 1], g[:, 1, 2], g[:, 2, 2] = m.T
    g[:, 1, 0], g[:, 2, 0], g[:, 2, 1] = m[:, 1], m[:, 2], m[:, 4]
    return g


def distance(a, b, h):
    """the largest difference of two results of `moments` on the same cloud: (centres / h, h G)"""
    return (float(np.abs(a["centres"].astype(np.float64) - b["centres"])[a["finite"]].max()) / h,
            float(np.abs(a["metric"].astype(np.float64) - b["metric"]).max()) * h)


def unit_extremes(kd, kg, q_min):
    """K_max and L = max q |K'| / K_max on [q_min, 1] for P and for P' (its derivative by differences on the same grid)"""
    q = np.unique(np.concatenate([np.linspace(min(q_min, 1.0), 1.0, 20001), [0.5]]))
    w, dw, g = np.abs(fr.W(kd, q, 1.0)), np.abs(fr.dW(kd, q, 1.0)), fr.dW(kg, q, 1.0)
    ddg = np.abs(np.gradient(g, q))
    w_max, g_max = float(w.max()), float(np.abs(g).max())
    return w_max, float((q * dw).max()) / w_max, g_max, float((q * ddg).max()) / g_max


def evaluate(points, centres, metric, mass, vol, kd=fr.CUBIC, kg=fr.CUBIC, chunk=1024):
    """points: (m, 3); centres (n, 3), metric (n, 6), mass and vol (n) of the particles; rows with a non-finite centre take no part.
    Float64 throughout; a point with a non-finite coordinate gets zeros."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    use = np.isfinite(c).all(axis=1)
    c, g = c[use], full(np.asarray(metric)[use])
    mass, vol = np.asarray(mass, np.float64)[use], np.asarray(vol, np.float64)[use]
    det = np.linalg.det(g)
    norm = np.linalg.eigvalsh(g)[:, -1]
    finite = np.isfinite(pts).all(axis=1)
    pi, pj, py, pq = [], [], [], []
    for a in range(0, len(pts), chunk):
        f = finite[a:a + chunk]
        p = np.where(f[:, None], pts[a:a + chunk], 0.0)
        d = p[:, None, :] - c[None, :, :]
        y = np.einsum("jkl,ijl->ijk", g, d)
        q = np.sqrt((y * y).sum(axis=2))
        i, j = np.nonzero((q <= 1.0) & f[:, None])
        pi.append(i + a); pj.append(j); py.append(y[i, j]); pq.append(q[i, j])
    i, j, y, q = np.concatenate(pi), np.concatenate(pj), np.concatenate(py), np.concatenate(pq)
    m = len(pts)
    q_min = float(q[q > 0.0].min()) if (q > 0.0).any() else 1.0
    w_max, w_l, g_max, g_l = unit_extremes(kd, kg, q_min)

    def total(values):
        return np.bincount(i, weights=values, minlength=m)

    w = fr.W(kd, q, 1.0)
    dw = np.where(q > fr.EPS, fr.dW(kg, q, 1.0), 0.0)
    z = np.einsum("pkl,pl->pk", g[j], y) / np.where(q > 0.0, q, 1.0)[:, None]
    return {"n": np.bincount(i, minlength=m).astype(np.int64), "density": total(mass[j] * det[j] * w), "fraction": total(vol[j] * det[j] * w),
            "gradient": np.stack([total(mass[j] * det[j] * dw * z[:, a]) for a in range(3)], axis=1),
            "A_density": total(mass[j] * det[j]) * w_max, "A_fraction": total(vol[j] * det[j]) * w_max,
            "A_gradient": total(mass[j] * det[j] * norm[j]) * g_max, "c_value": 16.0 + 92.0 * w_l + 320.0, "c_gradient": 476.0 + 92.0 * g_l,
            "q_min": q_min}


def tol_sum(n, A, c):
    """what a device sum may differ by"""
    return (np.asarray(n, np.float64) + c) * U * np.asarray(A, np.float64)


def compare(got, ref, fields=("density", "fraction", "gradient")):
    """Asserts the fields of `got` (flat arrays) against the reading at the derived tolerance; prints the worst error / tolerance."""
    m = len(ref["n"])
    empty = ref["n"] == 0
    for name in fields:
        if name not in got:
            continue
        g = np.asarray(got[name]).astype(np.float64).reshape(m, -1)
        r = np.asarray(ref[name], np.float64).reshape(m, -1)
        tol = tol_sum(ref["n"], ref["A_" + name], ref["c_gradient" if name == "gradient" else "c_value"])[:, None]
        assert np.isfinite(g).all(), name
        assert (g[empty] == 0.0).all(), (name, "not exactly zero where no particle reaches")
        err = np.abs(g - r)
        some = ~empty[:, None] & (tol > 0.0) & np.ones_like(err, bool)
        ratio = float((err[some] / np.broadcast_to(tol, err.shape)[some]).max()) if some.any() else 0.0
        print(f"{name}: worst error / tolerance = {ratio:.4f} over {int((~empty).sum())} places")
        worst = np.unravel_index(np.argmax(err - tol), err.shape)
        assert (err <= tol).all(), (name, worst, g[worst], r[worst], float(tol[worst[0], 0]), int(ref["n"][worst[0]]))


# ------------------------------------------------------------------------------------------------ the inputs
def separate(x, jitter, h, rng, margin=1.0e-4):
    """Re-jitters particles (x: f32 positions; jitter: (n, 3) half-widths per axis, the freedom each particle has) while any pair
    distance lies within margin * h of 2h: the f32 and the f64 neighbourhoods are then the same sets.  Returns the f32 positions."""
    x = np.asarray(x, F32).copy()
    base = x.astype(np.float64)
    for _ in range(200):
        bad = near_the_border(x, h, margin)
        if not len(bad):
            return x
        for k in np.unique(bad[:, 1]):
            x[k] = (base[k] + rng.uniform(-1.0, 1.0, 3) * jitter[k]).astype(F32)
    raise AssertionError("no separated cloud found")


def near_the_border(x, h, margin=1.0e-4):
    """the pairs (i < j) of finite rows whose distance lies within margin * h of 2h"""
    p = np.asarray(x, np.float64)
    ok = np.isfinite(p).all(axis=1)
    q = np.where(ok[:, None], p, 0.0)
    r = np.sqrt(((q[:, None, :] - q[None, :, :]) ** 2).sum(axis=2))
    i, j = np.nonzero((np.abs(r - 2.0 * h) <= margin * h) & ok[:, None] & ok[None, :])
    return np.stack([i[i < j], j[i < j]], axis=1)


def standard_cloud():
    """(a): §20's standard case (1 386 particles in two fluids), re-jittered by +-0.2 r where a pair sits on the border"""
    case = dict(fr.standard_case())
    n = len(case["x"])
    case["x"] = separate(case["x"], np.full((n, 3), 0.2 * case["r"]), case["h"], np.random.default_rng(23))
    return case


def lattice(nx, ny, nz, step):
    ix, iy, iz = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    return np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1) * step


def shapes_cloud(seed=29):
    """(b): at the standard r and h, each shape more than 4h from the next - a jittered 9 x 9 x 9 block, a one-particle-thick 15 x 15
    sheet (the k_r clamp is active), a single-file line of 15 (two equal small eigenvalues), a pair, a lone particle, 30 particles at one
    point (C = 0), one particle at NaN and one stray 10^4 h away.  One fluid; `parts` names the rows of each shape."""
    rng = np.random.default_rng(seed)
    r, h = fr.R, float(fr.H32)
    j = 0.2 * r
    pieces = [("block", lattice(9, 9, 9, 2.0 * r), (j, j, j)),
              ("sheet", lattice(15, 1, 15, 2.0 * r) + (1.5, 0.0, 0.0), (j, 0.02 * r, j)),
              ("line", lattice(15, 1, 1, 2.0 * r) + (0.0, 1.5, 0.0), (j, 0.0, 0.0)),
              ("pair", np.array([[0.0, 0.0, 1.5], [r, 0.0, 1.5]]), (0.0, 0.0, 0.0)),
              ("lone", np.array([[1.5, 1.5, 0.0]]), (0.0, 0.0, 0.0)),
              ("heap", np.repeat(np.array([[1.5, 0.0, 1.5]]), 30, axis=0), (0.0, 0.0, 0.0)),
              ("nan", np.array([[np.nan, 0.0, 0.0]]), (0.0, 0.0, 0.0)),
              ("stray", np.array([[1.0e4 * h, 0.0, 0.0]]), (0.0, 0.0, 0.0))]
    xs, js, parts, at = [], [], {}, 0
    for name, base, jit in pieces:
        jit = np.broadcast_to(np.asarray(jit, np.float64), base.shape)
        xs.append(base + rng.uniform(-1.0, 1.0, base.shape) * jit)
        js.append(jit)
        parts[name] = slice(at, at + len(base))
        at += len(base)
    x = separate(np.concatenate(xs).astype(F32), np.concatenate(js), h, rng)
    n = len(x)
    vol = (0.8 * (2.0 * r) ** 3 * (1.0 + 0.25 * np.arange(n) / n)).astype(F32)
    # places: around every shape, and a few nowhere
    near = np.concatenate([x[parts[k]][::3] for k in ("block", "sheet", "line", "pair", "lone", "heap")]).astype(np.float64)
    points = (near + rng.uniform(-1.2 * h, 1.2 * h, near.shape)).astype(F32)
    points = np.concatenate([points, F32([[5.0, 5.0, 5.0], [np.nan, 0.0, 0.0]])])
    return {"r": r, "h": h, "x": x, "vol": vol, "rho0": np.full(n, fr.DENSITY0[0]), "parts": parts, "points": points}


def rest_block(seed=31):
    """What the anisotropic kernels are for: a 12 x 8 x 12 block at rest, jittered by +-0.2 r, and a lattice at spacing r over the middle
    of its top face.  top_heights picks the vertices of a mesh that belong to that face."""
    rng = np.random.default_rng(seed)
    r, h = fr.R, float(fr.H32)
    base = lattice(12, 8, 12, 2.0 * r)
    x = separate((base + rng.uniform(-0.2 * r, 0.2 * r, base.shape)).astype(F32), np.full(base.shape, 0.2 * r), h, rng)
    top = 7 * 2.0 * r
    origin = F32([4.0 * r, top - 3.0 * r, 4.0 * r])
    return {"r": r, "h": h, "x": x, "vol": F32((2.0 * r) ** 3), "origin": origin, "spacing": F32(r), "dims": (15, 9, 15), "top": top}


def top_heights(vertices):
    return np.asarray(vertices, np.float64)[:, 1]
