"""The ray casts at the fluid (salva_hip_cast_rays / _cast_rays_camera) read from include/salva_hip.h, not from the
kernels: brute force over all rays x all particles in numpy f32, operation by operation.  No grid and no pruning; ties go to the
lower fluid slot, then the lower index (the particles are passed in host order, so that is the lower row); the thickness is summed
in f64 from the f32 chords.

`cast` is the reading.  `cast_f64` is the geometric ray / sphere intersection in f64, without the advance, for the CPU test that the
reading means what it says.  `walk_covers` is a small numpy model of the walk of salva_amd/csrc/fluidcast.hip, for the CPU test
that its margin eps really covers a case.

eps.  With M = the largest |coordinate| of G plus the sum of G's extents, every f32 quantity of a cast after the advance is at most M
in magnitude, so one rounding is at most U = 2^-24 M.  (a) ray_ball's p = q + tm d: q, the product and the sum round once each, 3 U
per component, at most 3 sqrt(3) U < 5.2 U as a vector - whatever tm is, since an error of tm only moves p along the ray; R R and the
dot add less than 1.5 U of R.  So a sphere that the f32 cast meets is met by the exact line through o' within R + 7 U, and its
computed entry and exit points lie within R + 8 U of its centre.  (b) The plane (float)cell * h rounds once (U), a particle's cell
along the dominant axis k is floor(fl(x / h)) (U), t = (plane - o'_k) / d_k and a(t) = o'_a + t d_a add 3 U propagated (|d_a / d_k|
<= 1) + 3 U of their own.  (c) Geometry: a centre c at distance <= rho from the line, and the line's point g at the same x_k: c - g
has no k component, and dist^2 = |c - g|^2 - ((c - g) . u)^2 >= |c - g|^2 (1 - (u_a^2 + u_b^2)) >= |c - g|^2 / 3 because u_k is the
largest component of the unit direction: |c_a - g_a| <= sqrt(3) rho.  With rho = R + 7 U that is < 1.75 R + 12.2 U.  (d) The
interval's ends and the cells of both sides use the same monotone floor(fl(x / h)): no further fuzz, one rounding of the subtraction
(U).  Sum: 12.2 + 6 + 1 + 1 (the k cell) + 1 < 22 U.  The walk uses eps = 32 U = 2^-19 M, dilates by 1.75 R + eps on the two other
axes and by R + eps along k.  (The dilation is sqrt(3) R, not R: a ray along (1, 1, 1) passes a centre at distance R whose offset in
the slice plane is 1.22 R on an axis.)"""
import numpy as np

from compound_cast_reading import ball_iv

F = np.float32
INF = F(np.inf)
NONE = np.uint32(0xFFFFFFFF)
R_PARTICLE = 0.025
H32 = F(F(R_PARTICLE) * F(2.0) * F(2.0))  # liquid_world.rs:44 in f32, as the library computes it
SIZES = (1500, 2603)


def _dot(a, b):
    return ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])


def bounds(x):
    """salva_hip_get_fluid_bounds: the box of the finite rows"""
    x = np.asarray(x, F).reshape(-1, 3)
    ok = np.isfinite(x).all(axis=1)
    if not ok.any():
        return None
    return x[ok].min(axis=0), x[ok].max(axis=0)


def counting(x, B):
    """1. the rows that count: finite and in B, faces included"""
    x = np.asarray(x, F).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return np.isfinite(x).all(axis=1) & (x >= B[0]).all(axis=1) & (x <= B[1]).all(axis=1)


def grown(B, R):
    return (B[0] - F(R)).astype(F), (B[1] + F(R)).astype(F)


def advance(o, d, G, tmax):
    """2. -> (live, ta, o')"""
    o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
    m = len(o)
    with np.errstate(all="ignore"):
        dd = _dot(d, d)
        live = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & np.isfinite(dd) & (dd > 0)
        e0, e1 = np.full(m, -INF, F), np.full(m, INF, F)
        for a in range(3):
            flat = d[:, a] == 0
            live &= ~flat | ((o[:, a] >= G[0][a]) & (o[:, a] <= G[1][a]))
            u, v = (G[0][a] - o[:, a]) / d[:, a], (G[1][a] - o[:, a]) / d[:, a]
            e0 = np.where(flat, e0, np.maximum(e0, np.minimum(u, v))).astype(F)
            e1 = np.where(flat, e1, np.minimum(e1, np.maximum(u, v))).astype(F)
        live &= (e0 <= e1) & ~(e1 < 0) & ~(e0 > F(tmax))
        ta = np.where(live, np.maximum(e0, F(0)), F(0)).astype(F)
        op = (o + (ta[:, None] * d)).astype(F)
    return live, ta, op


def camera_rays(cam):
    """6. -> (origins, directions), row iy * width + ix"""
    w, h = int(cam["width"]), int(cam["height"])
    ix, iy = np.arange(w, dtype=np.uint32).astype(F), np.arange(h, dtype=np.uint32).astype(F)
    su = (((ix + F(0.5)) * (F(2.0) / F(w))) - F(1.0)).astype(F)
    sv = (((iy + F(0.5)) * (F(2.0) / F(h))) - F(1.0)).astype(F)
    SU, SV = np.tile(su, h), np.repeat(sv, w)
    f, r, u = (np.asarray(cam[k], F).reshape(3) for k in ("forward", "right", "up"))
    d = ((f[None, :] + (SU[:, None] * r[None, :])) + (SV[:, None] * u[None, :])).astype(F)
    o = np.broadcast_to(np.asarray(cam["origin"], F).reshape(3), d.shape).copy()
    return o, d


def cast(o, d, x, slots, R, tmax=np.inf, clip=None, chunk=256):
    """x: the selected fluids' rows in host order (n x 3), slots[j] the fluid of row j.  -> dict: t, fluid, index, normal (f32),
    thickness (f64, from the f32 chords), n (particles the ray meets) and A (sum |chord|, f64) for the tolerance, row (the winner's
    row of x, -1: a miss)."""
    o, d, x = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3), np.asarray(x, F).reshape(-1, 3)
    slots = np.asarray(slots, np.uint32)
    m, R, tmax = len(o), F(R), F(tmax)
    index = np.zeros(len(x), np.uint32)
    for s in np.unique(slots):
        index[slots == s] = np.arange(int((slots == s).sum()), dtype=np.uint32)
    out = {"t": np.full(m, INF, F), "fluid": np.full(m, NONE, np.uint32), "index": np.full(m, NONE, np.uint32), "normal": np.zeros((m, 3), F),
           "thickness": np.zeros(m, np.float64), "n": np.zeros(m, np.int64), "A": np.zeros(m, np.float64), "row": np.full(m, -1, np.int64)}
    B = (np.asarray(clip[0], F), np.asarray(clip[1], F)) if clip is not None else bounds(x)
    if B is None:
        return out
    keep = counting(x, B)
    if not keep.any():
        return out
    rows = np.nonzero(keep)[0]
    xs = x[rows]
    live, ta, op = advance(o, d, grown(B, R), tmax)
    for b in range(0, m, chunk):
        sel = np.nonzero(live[b:b + chunk])[0] + b
        if not len(sel):
            continue
        k, n = len(sel), len(xs)
        q = (op[sel][:, None, :] - xs[None, :, :]).astype(F).reshape(-1, 3)
        dd = np.repeat(d[sel], n, axis=0)
        with np.errstate(all="ignore"):
            t0, t1 = ball_iv(q, dd, R)
            t0, t1 = t0.reshape(k, n), t1.reshape(k, n)
            tA = ta[sel][:, None]
            tj = (tA + np.maximum(t0, F(0))).astype(F)
            chord = np.maximum(F(0), np.minimum((tA + t1).astype(F), tmax) - tj).astype(F)
            hit = (t1 >= 0) & (tj <= tmax)
        out["thickness"][sel] = chord.astype(np.float64).sum(axis=1)
        out["A"][sel] = np.abs(chord.astype(np.float64)).sum(axis=1)
        out["n"][sel] = (t1 > -INF).sum(axis=1)
        cand = np.where(hit, tj, INF)
        win = cand.argmin(axis=1)  # (the first of equal values: the lower row)
        tw = cand[np.arange(k), win]
        got = tw < INF
        g, wn = sel[got], win[got]
        out["t"][g] = tw[got]
        out["row"][g] = rows[wn]
        out["fluid"][g] = slots[rows[wn]]
        out["index"][g] = index[rows[wn]]
        # 4. the normal
        qq = (op[g] - xs[wn]).astype(F)
        nn = (qq + ((tw[got] - ta[g]).astype(F)[:, None] * d[g])).astype(F)
        mx = np.abs(nn).max(axis=1) if len(g) else np.zeros(0, F)
        ok = (mx > 0) & np.isfinite(mx)
        with np.errstate(all="ignore"):
            s = (nn / mx[:, None]).astype(F)
            ln = np.sqrt(((s[:, 0] * s[:, 0]) + (s[:, 1] * s[:, 1])) + (s[:, 2] * s[:, 2])).astype(F)
            out["normal"][g] = np.where(ok[:, None], s / ln[:, None], F(0)).astype(F)
    return out


def thickness_tolerance(ref):
    """(n + 16) 2^-24 sum |chord|: DESIGN.md §20's bound for an f32 sum in another order"""
    return (ref["n"] + 16) * 2.0 ** -24 * ref["A"]


# ------------------------------------------------------------------------------------------------ the f64 geometric reading
def cast_f64(o, d, x, R):
    """Per ray and particle, straight from o in f64: (tm, p, t0, t1) with p the distance of the centre from the line, NaN entry / exit
    where p >= R."""
    o, d, x = (np.asarray(v, np.float64) for v in (o, d, x))
    q = o[:, None, :] - x[None, :, :]
    a = (d * d).sum(axis=1)[:, None]
    tm = -(q * d[:, None, :]).sum(axis=2) / a
    pv = q + tm[:, :, None] * d[:, None, :]
    p = np.sqrt((pv * pv).sum(axis=2))
    with np.errstate(invalid="ignore"):
        half = np.sqrt((R * R - p * p) / a)
    return tm, p, tm - half, tm + half


# ------------------------------------------------------------------------------------------------ the walk's model
def cast_eps(G):
    m = F(max(np.abs(G[0]).max(), np.abs(G[1]).max()))
    e = F(0)
    for a in range(3):
        e = F(e + F(G[1][a] - G[0][a]))
    return F(F(m + e) * F(2.0 ** -19))


def cell_of(v, h):
    with np.errstate(all="ignore"):
        return np.floor((np.asarray(v, F) / F(h)).astype(F)).astype(np.int64)


def walk_covers(o, d, x, R, h, chunk=256):
    """For every (ray, particle) pair that is a candidate of the f32 cast (disc > 0 and t1 >= 0), whether the walk of fluidcast.hip would visit the particle's cell:
    its slice along the dominant axis lies between the walk's first slice and the grid's face, and its cells on the two other axes lie
    in the slice's dilated interval.  -> (pairs met, pairs not covered)"""
    o, d, x = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3), np.asarray(x, F).reshape(-1, 3)
    R, h = F(R), F(h)
    B = bounds(x)
    G = grown(B, R)
    eps = cast_eps(G)
    reach, dil = F(R + eps), F(F(F(1.75) * R) + eps)
    live, ta, op = advance(o, d, G, np.inf)
    cells = cell_of(x, h)
    met = missed = 0
    for b in range(0, len(o), chunk):
        sel = np.nonzero(live[b:b + chunk])[0] + b
        if not len(sel):
            continue
        k, n = len(sel), len(x)
        q = (op[sel][:, None, :] - x[None, :, :]).astype(F).reshape(-1, 3)
        with np.errstate(all="ignore"):
            t0, t1 = ball_iv(q, np.repeat(d[sel], n, axis=0), R)
        ri, pj = np.nonzero(((t0 < INF) & (t1 >= 0)).reshape(k, n))
        if not len(ri):
            continue
        r = sel[ri]
        ad = np.abs(d[r])
        kk = np.where((ad[:, 0] >= ad[:, 1]) & (ad[:, 0] >= ad[:, 2]), 0, np.where(ad[:, 1] >= ad[:, 2], 1, 2))
        ar = np.arange(len(r))
        dk, pk = d[r][ar, kk], op[r][ar, kk]
        fwd = dk > 0
        s = cells[pj][ar, kk]
        s0 = cell_of(np.where(fwd, pk - reach, pk + reach).astype(F), h)
        ok = np.where(fwd, s >= s0, s <= s0)
        plo, phi = (s.astype(F) * h).astype(F), ((s + 1).astype(F) * h).astype(F)
        ua, ub = ((plo - pk) / dk).astype(F), ((phi - pk) / dk).astype(F)
        for off in (1, 2):
            ax = (kk + off) % 3
            da, pa = d[r][ar, ax], op[r][ar, ax]
            a0, a1 = (pa + (ua * da)).astype(F), (pa + (ub * da)).astype(F)
            lo, hi = cell_of((np.minimum(a0, a1) - dil).astype(F), h), cell_of((np.maximum(a0, a1) + dil).astype(F), h)
            c = cells[pj][ar, ax]
            ok &= (c >= lo) & (c <= hi)
        met += len(r)
        missed += int((~ok).sum())
    return met, missed


# ------------------------------------------------------------------------------------------------ the standard case
def standard_case(seed=5):
    """r = 0.025, h = 4 r.  4 103 particles on a 17 x 16 x 16 lattice at 2 r (its first 4 103 nodes, x slowest), jittered by +-0.3 r;
    fluid 0 the first 1 500, fluid 1 the other 2 603 (the sink tests' sizes).  4 096 rays: origins uniform in the box grown by its own
    size (inside and outside), aimed at points uniform in the box (the last quarter: in the box grown by its size), their directions
    scaled by 0.5 .. 2.  A 64 x 48 camera above the
    block looking down -z with a slight tilt."""
    rng = np.random.default_rng(seed)
    r = R_PARTICLE
    ix, iy, iz = np.meshgrid(np.arange(17), np.arange(16), np.arange(16), indexing="ij")
    cell = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1)[:sum(SIZES)]
    x = (cell * (2.0 * r) + rng.uniform(-0.3 * r, 0.3 * r, (len(cell), 3))).astype(F)
    slots = np.where(np.arange(len(x)) < SIZES[0], 0, 1).astype(np.uint32)
    lo, hi = x.min(axis=0).astype(np.float64), x.max(axis=0).astype(np.float64)
    size = hi - lo
    m = 4096
    origins = rng.uniform(lo - size, hi + size, (m, 3))
    targets = rng.uniform(lo, hi, (m, 3))
    targets[3 * m // 4:] = rng.uniform(lo - size, hi + size, (m - 3 * m // 4, 3))  # (the last quarter mostly misses)
    directions = (targets - origins) / np.linalg.norm(targets - origins, axis=1)[:, None] * rng.uniform(0.5, 2.0, (m, 1))
    mid = 0.5 * (lo + hi)
    camera = {"origin": np.array([mid[0], mid[1], hi[2] + 1.0], F), "forward": np.array([0.02, -0.01, -1.0], F),
              "right": np.array([0.55, 0.0, 0.011], F), "up": np.array([0.0, 0.42, -0.0042], F), "width": 64, "height": 48}
    return {"r": r, "h": float(H32), "x": x, "slots": slots, "n0": SIZES[0], "origins": origins.astype(F), "directions": directions.astype(F),
            "camera": camera, "radii": (r, 0.5 * float(H32) * 0.75)}


def make_world(x, slots, r=R_PARTICLE):
    """a world with the rows of x as fluids 0 .. max(slots), in host order"""
    from salva_amd import DFSPHSolver, Fluid, LiquidWorld

    w = LiquidWorld(DFSPHSolver(), r, 2.0)
    fluids = [w.add_fluid(Fluid(np.asarray(x, F)[np.asarray(slots) == s], r, 1000.0)) for s in range(int(np.max(slots)) + 1)]
    return w, fluids
