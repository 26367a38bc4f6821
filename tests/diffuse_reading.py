"""A brute-force reading of the potentials of diffuse particles (include/salva_hip.h "Diffuse particles"): plain numpy,
all pairs, no grid.  Written from the header's contract, not from the device code; the kernel gradient is tests/field_reading.py's.

`potentials` runs in float64, or in float32 throughout (dtype=numpy.float32) with every operation rounded as the header pins it; the
distance between the two runs on the same cloud is printed by tests/test_diffuse_cpu.py beside the tolerances below.

The tolerances are derived, not chosen.  u = 2^-24, one rounding of an f32 operation relative to its result.  A device sum of n terms
may differ from the reading by at most (n + c) u A: n - 1 roundings of an f32 sum in any order, each of a partial sum below A, and c for
one term.  As in tests/field_reading.py, A is in units of the largest magnitude a term can take and not of the term itself, because
the cancellations inside a term (1 - cosine, 1 - r / h, the kernel's (1 - q)^2) are absolute, not relative:

  trapped_air   term = (s (1 - c)) W_d <= 2 s, so A = sum_j 2 s_j with s_j = |v_ij|.  x_ij, v_ij: u per component.  |.|^2: 2u from the
                components, 1u the products, 2u the sums, halved by the root, 1u the root: s and r to 3.5u.  dot(v_ij, x_ij): 3u the
                factors and products, 2u the sums, of s r.  c = (dot / s) / r: 5u + 7u + 2u = 14u absolute; 1 - c: 2u more, 16u.
                W_d = 1 - r / h: 3.5u + 1u + 1u = 5.5u absolute.  The two products and s: 5.5u of the term.  Together
                s (16 + 2 x 5.5 + 2 x 5.5) u = 38u s = 19u (2 s): c = 20.
  g             the field evaluator's gradient with V_j for m_j: A = sum_j V_j G_max, G_max the largest |dW/dr| on [q_min, 1], c = 16
                (tests/field_reading.py), per component.
  normal        -g / |g|.  E = sqrt(3) (n + 16) u A bounds the error of g as a vector, and |a / |a| - b / |b|| <= |a - b| / min(|a|, |b|),
                so the device's normal lies within E / (|g| - E) + 4u of the reading's (the root, the quotient, |g|^2), as a vector.
                |g| >= surface_min / h where there is a normal at all: that floor is what keeps this bound small.
  wave_crest    compared with the reading FED THE DEVICE'S OWN NORMALS, so only the sum is under test.  term = (1 - min(dot(n_i, n_j), 1))
                W_d <= 2, so A = 2 (the number of terms).  dot of two unit vectors: 3u + 2u; 1 - dot: 2u more, 7u absolute; W_d 5.5u
                absolute; the product 1u of the term: 7u + 2 x 5.5u + 2u = 20u = 10u x 2: c = 10.

Discontinuous decisions.  Where the reading's value lies within the rounding of a test's two sides, the device may decide either way,
and the row's bound is widened by exactly the terms at stake (`wide` marks such rows; the inputs are chosen so that they are at most
1 % of a cloud):
  |x_ij|^2 <= h^2      never at stake: the clouds are re-jittered until no pair lies within 1e-4 h of h, so `count` is exact.
  dot(x_ij, n_i) > 0   1u per component of x_ij, 1u per product, 2u the sums: at stake when |dot| <= 8u |x_ij|; the term is added to
                       the row's bound.
  h |g| >= surface_min at stake when |h |g| - surface_min| <= h E + 4u surface_min: the zero vector and the normal both pass.
  v.n / |v| >= crest_cos   v and n are the device's own: 3u the products, 2u the sums, 2.5u the root, 1u the quotient, of at most 1:
                       at stake when |cos - crest_cos| <= 10u; 0 and kappa both pass.

The set (advect, remove, emit) is restated in f32 operation for operation - `advect` and `emit` below - and compared bit for bit: it is
fed what the device itself returned (the evaluator's count and velocity at the diffuse particles; the potentials), so nothing with a
tolerance enters.

Test infrastructure only."""
from dataclasses import dataclass

import numpy as np

import field_reading as fr

F32 = np.float32
U = fr.U
C_TRAPPED, C_GRADIENT, C_CREST = 20.0, 16.0, 10.0
SIGN_MARGIN, COS_MARGIN = 8.0 * U, 10.0 * U


@dataclass
class Params:
    """SalvaHipDiffuse under the names of salva_amd.Diffuse; the defaults are salva_hip_default_diffuse's"""
    surface_min: float = 0.25
    crest_cos: float = 0.6
    trapped_air: tuple = (5.0, 20.0)
    wave_crest: tuple = (2.0, 8.0)
    energy: tuple = (5.0, 50.0)
    k_ta: float = 4000.0
    k_wc: float = 50000.0
    max_per_particle: int = 16
    n_spray: int = 6
    n_bubble: int = 20
    k_b: float = 2.0
    k_d: float = 0.8
    lifetime: tuple = (2.0, 5.0)
    seed: int = 0
    kill_box: object = None
    gravity: tuple = (0.0, -9.81, 0.0)


def dot(a, b):
    """((ax bx) + (ay by)) + (az bz) in the arrays' own type, along the last axis"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _inputs(x, v, vol, rho0, h, T):
    x, v = np.asarray(x, T).reshape(-1, 3), np.asarray(v, T).reshape(-1, 3)
    n = len(x)
    vol = np.broadcast_to(np.asarray(vol, F32), (n,))
    mass = (vol * np.broadcast_to(np.asarray(rho0, np.float64).astype(F32), (n,))).astype(F32)  # one f32 product
    finite = np.isfinite(x).all(axis=1)
    h32 = F32(h)
    h2 = T(h32 * h32) if T is F32 else T(h32) * T(h32)
    return x, v, vol.astype(T), mass.astype(T), finite, T(h32), h2


def potentials(x, v, vol, rho0, h, p=None, dtype=np.float64, kg=fr.CUBIC):
    """x, v: (n, 3); vol, rho0: (n) or scalars - rho0 the rest density of each particle's fluid.  Returns a dict of arrays in `dtype`:
    count, trapped_air, g (n, 3), gnorm, normal (n, 3), energy, and for the tolerances n (= count), A_trapped, A_gradient; a non-finite
    row is all zeros.  The wave crest is `crest`'s, which takes the normals it is to use."""
    p = p or Params()
    T = dtype
    x, v, vol, mass, finite, h, h2 = _inputs(x, v, vol, rho0, h, T)
    n = len(x)
    xs = np.where(finite[:, None], x, T(0))
    count, ta, g = np.zeros(n, np.int64), np.zeros(n, T), np.zeros((n, 3), T)
    a_ta, a_g, r_min = np.zeros(n), np.zeros(n), np.inf
    idx = np.arange(n)
    pairs = []
    for i in np.nonzero(finite)[0]:
        d = (xs[i] - xs).astype(T)
        r2 = dot(d, d)
        near = np.nonzero(finite & (r2 <= h2) & (idx != i))[0]
        d, r2 = d[near], r2[near]
        r = np.sqrt(r2)
        count[i] = len(near)
        w = (v[i] - v[near]).astype(T)
        ww = dot(w, w)
        ok = (ww > 0) & (r2 > 0)
        s, rr = np.sqrt(np.where(ok, ww, T(1))), np.where(ok, r, T(1))
        c = np.clip((dot(w, d) / s) / rr, T(-1), T(1))
        term = np.where(ok, (s * (T(1) - c)) * (T(1) - r / h), T(0)).astype(T)
        ta[i] = term.sum(dtype=T)
        a_ta[i] = float(np.where(ok, 2.0 * s, 0.0).sum())
        # the header's two zero rules: r <= eps here, and r <= 1e-5 h for the cubic spline inside fr.dW (the `close` pair of the shapes)
        with np.errstate(divide="ignore", invalid="ignore"):
            gfac = np.where(r > fr.EPS, fr.dW(kg, r.astype(np.float64), float(h)) / np.where(r > 0, r, 1).astype(np.float64), 0.0).astype(T)
        g[i] = ((vol[near] * gfac)[:, None] * d).sum(axis=0, dtype=T)
        a_g[i] = float(vol[near].sum())
        if len(near):
            r_min = min(r_min, float(r.min()))
        pairs.append((i, near))
    gnorm = np.sqrt(dot(g, g))
    has = finite & (gnorm > 0) & (h * gnorm >= T(p.surface_min))
    normal = np.where(has[:, None], -g / np.where(has, gnorm, T(1))[:, None], T(0)).astype(T)
    energy = np.where(finite, (T(0.5) * mass) * dot(v, v), T(0)).astype(T)
    q_min = min(r_min / float(h), 1.0) if np.isfinite(r_min) else 1.0
    return {"count": count, "n": count, "trapped_air": ta, "g": g, "gnorm": gnorm, "normal": normal, "has_normal": has, "energy": energy,
            "A_trapped": a_ta, "A_gradient": a_g * fr.k_max(fr.dW, kg, float(h), q_min), "finite": finite, "h": float(h)}


def crest(x, v, h, normals, p=None, dtype=np.float64):
    """The wave crest with the normals as given ((n, 3); a zero row: no normal).  Returns kappa (gated), and for the tolerances n (the
    number of terms), at_stake (the terms whose sign test is within SIGN_MARGIN), close (the gate is within COS_MARGIN) and open (the
    sum without the gate)."""
    p = p or Params()
    T = dtype
    x, v, _, _, finite, h, h2 = _inputs(x, v, 1.0, 1.0, h, T)
    nrm = np.asarray(normals, T).reshape(-1, 3)
    n = len(x)
    has = finite & (nrm != 0).any(axis=1)
    xs = np.where(finite[:, None], x, T(0))
    idx = np.arange(n)
    kappa, opened, terms, stake, close = np.zeros(n, T), np.zeros(n, T), np.zeros(n, np.int64), np.zeros(n), np.zeros(n, bool)
    for i in np.nonzero(has)[0]:
        vv = dot(v[i], v[i])
        if not vv > 0:
            continue
        cosine = dot(v[i], nrm[i]) / np.sqrt(vv)
        close[i] = abs(float(cosine) - float(F32(p.crest_cos))) <= COS_MARGIN
        d = (xs[i] - xs).astype(T)
        r2 = dot(d, d)
        sign = dot(d, np.broadcast_to(nrm[i], d.shape))
        near = finite & (r2 <= h2) & (idx != i) & has
        take = np.nonzero(near & (sign > 0))[0]
        term = ((T(1) - np.minimum(dot(np.broadcast_to(nrm[i], (len(take), 3)), nrm[take]), T(1))) * (T(1) - np.sqrt(r2[take]) / h)).astype(T)
        opened[i] = term.sum(dtype=T)
        terms[i] = len(take)
        edge = np.nonzero(near & (np.abs(sign) <= SIGN_MARGIN * np.sqrt(r2)))[0]
        if len(edge):
            stake[i] = float(((1.0 - np.minimum(dot(np.broadcast_to(nrm[i], (len(edge), 3)), nrm[edge]), 1.0)) * (1.0 - np.sqrt(r2[edge]) / h)).sum())
        if cosine >= T(F32(p.crest_cos)):
            kappa[i] = opened[i]
    return {"wave_crest": kappa, "open": opened, "n": terms, "at_stake": stake, "close": close}


def tol_sum(n, A, c):
    """what a device sum may differ by"""
    return (np.asarray(n, np.float64) + c) * U * np.asarray(A, np.float64)


def normal_bounds(ref, p=None):
    """per row: the bound on |n_device - n_reading| as a vector, and whether the decision h |g| >= surface_min is at stake"""
    p = p or Params()
    e = np.sqrt(3.0) * tol_sum(ref["n"], ref["A_gradient"], C_GRADIENT)
    gn = np.asarray(ref["gnorm"], np.float64)
    # (e = 0: a row without neighbours has g = 0 on both sides and nothing to decide)
    wide = ref["finite"] & (e > 0) & (np.abs(ref["h"] * gn - p.surface_min) <= ref["h"] * e + 4.0 * U * p.surface_min)
    with np.errstate(divide="ignore", invalid="ignore"):
        tol = np.where(gn > e, e / (gn - e), np.inf) + 4.0 * U
    return tol, wide


def compare(got, ref, p=None):
    """count, trapped_air, energy and normal of the device (`got`: flat arrays) against the f64 reading `ref`; prints the worst fraction
    of each bound first.  Returns the rows whose normal decision was at stake."""
    p = p or Params()
    assert np.array_equal(np.asarray(got["count"]).astype(np.int64), ref["count"]), "count"
    ta = np.asarray(got["trapped_air"], np.float64)
    tol = tol_sum(ref["n"], ref["A_trapped"], C_TRAPPED)
    err = np.abs(ta - ref["trapped_air"])
    some = tol > 0
    print(f"trapped_air: worst error / tolerance = {float((err[some] / tol[some]).max()) if some.any() else 0.0:.4f} over {int(some.sum())} rows")
    assert np.isfinite(ta).all() and (ta[~some] == 0).all() and (err <= tol).all(), ("trapped_air", int(np.argmax(err - tol)))
    # energy: |v|^2 to 3u, the two products 2u, m given
    en = np.asarray(got["energy"], np.float64)
    err, tol = np.abs(en - ref["energy"]), 5.0 * U * np.abs(ref["energy"])
    print(f"energy: worst error / tolerance = {float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0:.4f}")
    assert (err <= tol).all(), ("energy", int(np.argmax(err - tol)))
    nrm = np.asarray(got["normal"], np.float64).reshape(-1, 3)
    tol, wide = normal_bounds(ref, p)
    zero = (nrm == 0).all(axis=1)
    err = np.sqrt(((nrm - ref["normal"]) ** 2).sum(axis=1))
    want = ref["has_normal"]
    sure = ~wide
    assert np.array_equal(zero[sure], ~want[sure]), "which rows have a normal"
    both = ~zero & want
    print(f"normal: worst error / tolerance = {float((err[both] / tol[both]).max()) if both.any() else 0.0:.4f} over {int(both.sum())} rows, "
          f"{int(wide.sum())} decisions at stake")
    assert (err[both] <= tol[both]).all(), ("normal", int(np.argmax(np.where(both, err - tol, -np.inf))))
    # a row at stake that decided the other way: its normal is the direction of g all the same
    other = ~zero & ~want
    if other.any():
        g = ref["g"][other]
        assert (np.sqrt(((nrm[other] + g / np.sqrt((g * g).sum(axis=1))[:, None]) ** 2).sum(axis=1)) <= tol[other]).all()
    return wide


def compare_crest(got_crest, ref):
    """the device's wave crest against `crest` fed the device's normals; returns the rows whose bound was widened"""
    k = np.asarray(got_crest, np.float64)
    tol = tol_sum(ref["n"], 2.0 * ref["n"], C_CREST) + ref["at_stake"]
    wide = (ref["at_stake"] > 0) | ref["close"]
    r = np.asarray(ref["wave_crest"], np.float64)
    err = np.abs(k - r)
    either = ref["close"] & (np.abs(k - np.where(r == 0, ref["open"], 0.0)) <= tol)  # the gate decided the other way
    some = (tol > 0) & ~either
    print(f"wave_crest: worst error / tolerance = {float((err[some] / tol[some]).max()) if some.any() else 0.0:.4f} over {int((r > 0).sum())} crests, "
          f"{int(wide.sum())} rows widened")
    assert np.isfinite(k).all() and ((err <= tol) | either).all(), ("wave_crest", int(np.argmax(err - tol)))
    return wide


# ------------------------------------------------------------------------------------------------ the inputs
def near_the_border(x, h, margin=1.0e-4):
    """the pairs (i < j) of finite rows whose distance lies within margin * h of h"""
    q = np.asarray(x, np.float64)
    ok = np.isfinite(q).all(axis=1)
    q = np.where(ok[:, None], q, 0.0)
    r = np.sqrt(((q[:, None, :] - q[None, :, :]) ** 2).sum(axis=2))
    i, j = np.nonzero((np.abs(r - h) <= margin * h) & ok[:, None] & ok[None, :])
    return np.stack([i[i < j], j[i < j]], axis=1)


def separate(x, jitter, h, rng, margin=1.0e-4):
    """Re-jitters particles (x: f32 positions; jitter: (n, 3) half-widths per axis, the freedom each particle has) while any pair
    distance lies within margin * h of h: the f32 and the f64 neighbourhoods are then the same sets (DESIGN.md §23's device)."""
    x = np.asarray(x, F32).copy()
    base = x.astype(np.float64)
    for _ in range(200):
        bad = near_the_border(x, h, margin)
        if not len(bad):
            return x
        for k in np.unique(bad[:, 1]):
            if not jitter[k].any():
                k = bad[bad[:, 1] == k][0, 0]
            x[k] = (base[k] + rng.uniform(-1.0, 1.0, 3) * jitter[k]).astype(F32)
    raise AssertionError("no separated cloud found")


def flow(x, scale=1.0):
    """shear in x along y, and the whole cloud moving outwards from its centre: trapped air inside, crests on the faces"""
    q = np.asarray(x, np.float64)
    ok = np.isfinite(q).all(axis=1)
    centre, half = q[ok].mean(axis=0), max(float(np.ptp(q[ok], axis=0).max()) / 2.0, 1.0e-3)
    u = (q - centre) / half
    i = np.arange(len(q))
    v = 2.0 * u + np.stack([3.0 * u[:, 1] ** 2, 0.4 * np.sin(0.7 * i), 1.5 * u[:, 0] * u[:, 1]], axis=1)
    return (scale * np.where(ok[:, None], v, 0.0)).astype(F32)


def standard_cloud():
    """§20's standard case (1 386 particles in two fluids), re-jittered by +-0.2 r where a pair sits on the border, with `flow`"""
    case = dict(fr.standard_case())
    n = len(case["x"])
    case["x"] = separate(case["x"], np.full((n, 3), 0.2 * case["r"]), case["h"], np.random.default_rng(24))
    case["v"] = flow(case["x"])
    return case


def lattice(nx, ny, nz, step):
    ix, iy, iz = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    return np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1) * step


def shapes_cloud(seed=41):
    """At the standard r and h, each shape more than 2h from the next: a jittered 7 x 7 x 7 block with one particle at rest in its
    middle, a one-particle-thick 13 x 13 sheet, a single-file line of 15, a pair, a lone particle, two particles at the same place, two 2^-21 apart (above the
    reference's eps and below 1e-5 h: the cubic spline's gradient is zero there, W_d is not), one particle at NaN and one stray 2 000 h away.  One fluid; `parts` names the rows of each shape."""
    rng = np.random.default_rng(seed)
    r, h = fr.R, float(fr.H32)
    j = 0.2 * r
    pieces = [("block", lattice(7, 7, 7, 2.0 * r), (j, j, j)),
              ("sheet", lattice(13, 1, 13, 2.0 * r) + (1.0, 0.0, 0.0), (j, 0.02 * r, j)),
              ("line", lattice(15, 1, 1, 2.0 * r) + (0.0, 1.0, 0.0), (j, 0.0, 0.0)),
              ("pair", np.array([[0.0, 0.0, 1.0], [r, 0.0, 1.0]]), (0.0, 0.0, 0.0)),
              ("lone", np.array([[1.0, 1.0, 0.0]]), (0.0, 0.0, 0.0)),
              ("same", np.repeat(np.array([[1.0, 0.0, 1.0]]), 2, axis=0), (0.0, 0.0, 0.0)),
              ("close", np.array([[0.5, 1.5, 1.0], [0.5 + 2.0 ** -21, 1.5, 1.0]]), (0.0, 0.0, 0.0)),
              ("nan", np.array([[np.nan, 0.0, 0.0]]), (0.0, 0.0, 0.0)),
              ("stray", np.array([[2.0e3 * h, 0.0, 0.0]]), (0.0, 0.0, 0.0))]
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
    v = np.zeros((n, 3), F32)
    for name in ("block", "sheet", "line"):
        v[parts[name]] = flow(x[parts[name]])
    v[parts["pair"]] = F32([[-1.0, 0.5, 0.0], [1.0, 0.0, 0.25]])
    v[parts["lone"]] = F32([0.3, 0.2, 0.1])
    v[parts["same"]] = F32([[0.0, 1.0, 0.0], [0.0, -1.0, 0.5]])
    v[parts["close"]] = F32([[0.5, 0.0, 0.0], [-0.5, 0.25, 0.0]])
    rest = parts["block"].start + (3 * 7 + 3) * 7 + 3  # the middle of the block
    v[rest] = 0.0
    return {"r": r, "h": h, "x": x, "v": v, "vol": vol, "rho0": np.full(n, fr.DENSITY0[0]), "parts": parts, "rest": rest}


# ------------------------------------------------------------------------------------------------ the set, in f32, bit for bit
M32 = 0xFFFFFFFF
SPRAY, FOAM, BUBBLE, NEW = 0, 1, 2, 3


def fmix(x):
    """the header's mixing function, on Python integers or numpy uint64 arrays holding u32 values"""
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def key(seed, updates, slot, index):
    return fmix((fmix((fmix((fmix(seed & M32) + updates) & M32) + slot) & M32) + index) & M32)


def bits(seed, updates, slot, index, draw):
    return fmix((key(seed, updates, slot, index) + draw) & M32)


def uniform(k, draw):
    """u(d) = (float)(bits >> 8) * 2^-24 from a row's key"""
    return F32(fmix((k + draw) & M32) >> 8) * F32(2.0 ** -24)


def disc(k, d):
    """the header's rejection: at most eight attempts at draws d + 2t, d + 2t + 1, then (0, 0)"""
    for t in range(8):
        a = F32(2.0) * uniform(k, d + 2 * t) - F32(1.0)
        b = F32(2.0) * uniform(k, d + 2 * t + 1) - F32(1.0)
        if a * a + b * b <= F32(1.0):
            return a, b
    return F32(0.0), F32(0.0)


def phi(value, lo, hi):
    """Phi(I, lo, hi) = (min(I, hi) - min(I, lo)) / (hi - lo), in f32"""
    value, lo, hi = np.asarray(value, F32), F32(lo), F32(hi)
    return ((np.minimum(value, hi) - np.minimum(value, lo)) / F32(hi - lo)).astype(F32)


def advect(x, v, life, ids, count, vf, p, dt):
    """a. and b. of salva_hip_update_diffuse on f32 arrays; count, vf: the evaluator's `count` and `velocity` at x.  Returns the
    survivors (positions, velocities, lifetime, kind, id) and (dissolved, killed)."""
    x, v, life, vf = np.asarray(x, F32).reshape(-1, 3), np.asarray(v, F32).reshape(-1, 3), np.asarray(life, F32), np.asarray(vf, F32).reshape(-1, 3)
    count, dt, g = np.asarray(count, np.int64), F32(dt), np.asarray(p.gravity, F32)
    spray, bubble = count < p.n_spray, count > p.n_bubble
    foam = ~spray & ~bubble
    v_spray = v + (dt * g)[None, :]
    v_bubble = (v - ((dt * F32(p.k_b)) * g)[None, :]) + F32(p.k_d) * (vf - v)
    nv = np.where(spray[:, None], v_spray, np.where(foam[:, None], vf, v_bubble)).astype(F32)
    nlife = np.where(foam, life - dt, life).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        nx = (x + dt * nv).astype(F32)
    kind = np.where(spray, SPRAY, np.where(foam, FOAM, BUBBLE)).astype(np.uint32)
    killed = ~np.isfinite(nx).all(axis=1)
    if p.kill_box is not None:
        lo, hi = np.asarray(p.kill_box[0], F32), np.asarray(p.kill_box[1], F32)
        with np.errstate(invalid="ignore"):
            killed |= ((nx < lo) | (nx > hi)).any(axis=1)
    dissolved = ~killed & (nlife <= 0)
    keep = ~killed & ~dissolved
    return ({"positions": nx[keep], "velocities": nv[keep], "lifetime": nlife[keep], "kind": kind[keep], "id": np.asarray(ids, np.uint32)[keep]},
            (int(dissolved.sum()), int(killed.sum())))


def emission_counts(x, v, slot, index, pot, p, dt, updates):
    """c_i per row of the potentials call (x, v: the fluids' rows in that order; slot, index: each row's fluid and index within it;
    pot: the device's own trapped_air, wave_crest, energy)"""
    x, v, dt = np.asarray(x, F32).reshape(-1, 3), np.asarray(v, F32).reshape(-1, 3), F32(dt)
    rate = ((phi(pot["energy"], *p.energy) * (F32(p.k_ta) * phi(pot["trapped_air"], *p.trapped_air) + F32(p.k_wc) * phi(pot["wave_crest"], *p.wave_crest)))
            * dt).astype(F32)
    k = key(int(p.seed), int(updates), np.asarray(slot, np.uint64), np.asarray(index, np.uint64))
    u0 = ((fmix(k & M32) >> 8).astype(F32) * F32(2.0 ** -24)).astype(F32)  # (draw 0)
    t = (rate + u0).astype(F32)
    ok = np.isfinite(x).all(axis=1) & (dot(v, v) > 0) & (t >= 1)
    return np.where(ok, np.minimum(np.floor(t), F32(p.max_per_particle)), 0).astype(np.int64), k


def frame(v):
    """the header's orthonormal pair normal to v (f32 scalars)"""
    s = np.sqrt(dot(v, v))
    w = (v / s).astype(F32)
    a = np.abs(w)
    m = 0 if (a[0] <= a[1] and a[0] <= a[2]) else (1 if a[1] <= a[2] else 2)
    t = np.zeros(3, F32)
    t[m] = 1.0

    def cross(p, q):
        return np.array([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]], F32)

    c = cross(w, t)
    e1 = (c / np.sqrt(dot(c, c))).astype(F32)
    return e1, cross(w, e1)


def emit(x, v, slot, index, pot, p, dt, updates, radius, first_id, room):
    """c. of salva_hip_update_diffuse: the new particles in order (the first `room` of them) and (emitted, dropped)"""
    x, v = np.asarray(x, F32).reshape(-1, 3), np.asarray(v, F32).reshape(-1, 3)
    c, keys = emission_counts(x, v, slot, index, pot, p, dt, updates)
    total = int(c.sum())
    emitted = min(total, int(room))
    pos, vel, life = [], [], []
    dt, radius, lo, hi = F32(dt), F32(radius), F32(p.lifetime[0]), F32(p.lifetime[1])
    for i in np.nonzero(c)[0]:
        if len(pos) >= emitted:
            break
        e1, e2 = frame(v[i])
        k = int(keys[i])
        for j in range(int(c[i])):
            if len(pos) >= emitted:
                break
            d = 1 + 20 * j
            a, b = disc(k, d)
            cc = uniform(k, d + 16) * dt
            pos.append((x[i] + radius * (a * e1 + b * e2)) + cc * v[i])
            vel.append(v[i])
            life.append(lo + uniform(k, d + 17) * F32(hi - lo))
    new = {"positions": np.array(pos, F32).reshape(-1, 3), "velocities": np.array(vel, F32).reshape(-1, 3), "lifetime": np.array(life, F32),
           "kind": np.full(emitted, NEW, np.uint32), "id": (np.uint32(first_id) + np.arange(emitted, dtype=np.uint32)).astype(np.uint32)}
    return new, (emitted, total - emitted), c


def rows_of(case_slots):
    """slot and index within the fluid of each packed row, from the fluids' lengths by ascending slot: [(slot, n), ...]"""
    slot = np.concatenate([np.full(n, s, np.uint64) for s, n in case_slots])
    index = np.concatenate([np.arange(n, dtype=np.uint64) for _, n in case_slots])
    return slot, index
