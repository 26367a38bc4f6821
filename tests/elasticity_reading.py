"""A numpy reading of Becker2009Elasticity (solver/elasticity/becker2009_elasticity.rs), written from the reference's semantics:
float64 inside, f32 epsilon and 20 iterations in the rotation extraction, vectorised over particles (CSR + einsum / bincount).

`rotation_from_matrix_eps`, `rotations_and_stresses` and `accelerations` take a `dtype`.  With np.float32 every array they touch is
f32, so every sum, product, division, square root, sine and cosine rounds to f32 (numpy never widens an f32 ufunc; Python scalars
are weak under NEP 50, which numpy >= 2 implements); the neighbour sums add contact by contact in row order.  The distance between
that replay and the float64 reading is the noise floor the device is held to (tests/test_elasticity_reading_cpu.py).

`ElasticityReading(E, nu, nonlinear)` keeps the force's state (positions0, contacts0, volumes0, rotations, ...) like the reference
and has the `solve(...)` of a NonPressureForce, so it runs as a host force of a LiquidWorld (SALVA_HIP_FORCE_CUSTOM) or of the CPU
checker.  Test infrastructure only."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
CUBIC, POLY6, SPIKY, VISCOSITY = 0, 1, 2, 3


def kernel_w(r, h, kind=CUBIC, dtype=np.float64):
    """KernelDensity::scalar_apply (kernel/*_kernel.rs, dim3)."""
    r, h = np.asarray(r, dtype), float(h)
    if kind == CUBIC:
        q = r / h
        inner = 1.0 + (q * q * q - q * q) * 6.0
        outer = (1.0 - q) ** 3 * 2.0
        return 8.0 / (np.pi * h ** 3) * np.where(q <= 0.5, inner, np.where(q <= 1.0, outer, 0.0))
    if kind == POLY6:
        return np.where(r <= h, 315.0 / (64.0 * np.pi * h ** 9) * (h * h - r * r) ** 3, 0.0)
    if kind == SPIKY:
        return np.where(r <= h, 15.0 / (np.pi * h ** 6) * (h - r) ** 3, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = 15.0 / (2.0 * np.pi * h ** 3) * (r * r / (h * h) * (1.0 - r / (2.0 * h)) + h / (2.0 * r) - 1.0)
    return np.where((r <= h) & (r > 0.0), v, 0.0)


def kernel_dw(r, h, kind=CUBIC, dtype=np.float64):
    """KernelGradient::scalar_apply_diff."""
    r, h = np.asarray(r, dtype), float(h)
    if kind == CUBIC:
        q = r / h
        inner = (q * 3.0 - 2.0) * q * 6.0
        outer = -(1.0 - q) ** 2 * 6.0
        v = np.where((q > 1.0) | (q <= 1.0e-5), 0.0, np.where(q <= 0.5, inner, outer))
        return 8.0 / (np.pi * h ** 3) * v / h
    if kind == POLY6:
        return np.where(r <= h, 315.0 / (64.0 * np.pi * h ** 9) * (h * h - r * r) ** 2 * r * -6.0, 0.0)
    if kind == SPIKY:
        return np.where(r <= h, -15.0 / (np.pi * h ** 6) * (h - r) ** 2 * 3.0, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = 15.0 / (2.0 * np.pi * h ** 3) * (-3.0 * r * r / (2.0 * h ** 3) + 2.0 * r / (h * h) - h / (2.0 * r * r))
    return np.where((r <= h) & (r > 0.0), v, 0.0)


def norm(v, dtype=np.float64):
    """|v| along the last axis as sqrt((x x + y y) + z z), every step in `dtype`."""
    v = np.asarray(v, dtype)
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def gradient(d, h, kind=CUBIC, dtype=np.float64):
    """Kernel::apply_diff1(v) (kernel.rs:18-24): (v / |v|) dW/dr, zero when |v| <= eps."""
    d = np.asarray(d, dtype)
    r = norm(d, dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(r > EPS32, kernel_dw(r, h, kind, dtype) / r, dtype(0.0))
    return d * f[..., None]


def dist2_f32(a, b):
    """|a - b|^2 rounded like nalgebra's f32 norm_squared: ((dx dx + dy dy) + dz dz), no fused operations."""
    d = (np.asarray(a, np.float32) - np.asarray(b, np.float32)).astype(np.float32)
    s = (d[..., 0] * d[..., 0]).astype(np.float32) + (d[..., 1] * d[..., 1]).astype(np.float32)
    return (s.astype(np.float32) + (d[..., 2] * d[..., 2]).astype(np.float32)).astype(np.float32)


def rest_contacts(p0, h):
    """compute_self_contacts (contacts.rs:403-446): every ordered pair of the fluid with d^2 <= h^2 in f32, self pairs included.
    CSR (offsets, j), rows ascending in j."""
    from scipy.spatial import cKDTree

    p0 = np.asarray(p0, np.float32)
    n = len(p0)
    h32 = np.float32(h)
    pairs = cKDTree(p0.astype(np.float64)).query_pairs(float(h) * (1.0 + 1e-4), output_type="ndarray")
    if len(pairs):
        keep = dist2_f32(p0[pairs[:, 0]], p0[pairs[:, 1]]) <= np.float32(h32 * h32)
        pairs = pairs[keep]
    self_ = np.arange(n)
    i = np.concatenate([pairs[:, 0], pairs[:, 1], self_]) if len(pairs) else self_
    j = np.concatenate([pairs[:, 1], pairs[:, 0], self_]) if len(pairs) else self_
    order = np.lexsort((j, i))
    i, j = i[order], j[order]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(i, minlength=n), out=off[1:])
    return off, j


def rows(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def coefficients(E, nu):
    """elasticity_coefficients (:15-24)."""
    d0 = E * (1.0 - nu) / ((1.0 + nu) * (1.0 - 2.0 * nu))
    d1 = E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
    d2 = E * (1.0 - 2.0 * nu) / (2.0 * (1.0 + nu) * (1.0 - 2.0 * nu))
    return d0, d1, d2


def rotation_from_matrix_eps(A, R, eps=EPS32, max_iter=20, dtype=np.float64):
    """Rotation3::from_matrix_eps (nalgebra; Mueller et al. 2016) for a stack of matrices, warm-started from R."""
    A = np.asarray(A, dtype)
    R = np.array(R, dtype)
    eps = float(eps)
    active = np.ones(len(A), bool)
    for _ in range(max_iter):
        if not active.any():
            break
        w = np.cross(R[:, :, 0], A[:, :, 0]) + np.cross(R[:, :, 1], A[:, :, 1]) + np.cross(R[:, :, 2], A[:, :, 2])
        den = np.einsum("nrc,nrc->n", R, A)
        w = w / (np.abs(den) + eps)[:, None]
        ang = norm(w, dtype)
        active &= ang > eps
        if not active.any():
            break
        u = w[active] / ang[active, None]
        a = ang[active]
        s, c = np.sin(a), np.cos(a)
        K = np.zeros((len(a), 3, 3), dtype)
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -u[:, 2], u[:, 1], -u[:, 0]
        K[:, 1, 0], K[:, 2, 0], K[:, 2, 1] = u[:, 2], -u[:, 1], u[:, 0]
        Q = np.eye(3, dtype=dtype) * c[:, None, None] + s[:, None, None] * K + (1.0 - c)[:, None, None] * np.einsum("ni,nj->nij", u, u)
        R[active] = np.einsum("nij,njk->nik", Q, R[active])
    return R


def sym_mul(s, v):
    """sym_mat_mul_vec (:27-37) on stacks: s = (xx, yy, zz, xy, xz, yz)."""
    return np.stack([s[:, 0] * v[:, 0] + s[:, 3] * v[:, 1] + s[:, 4] * v[:, 2],
                     s[:, 3] * v[:, 0] + s[:, 1] * v[:, 1] + s[:, 5] * v[:, 2],
                     s[:, 4] * v[:, 0] + s[:, 5] * v[:, 1] + s[:, 2] * v[:, 2]], axis=1)


def segsum(ci, vals, n):
    """sum of per-contact rows into their particles (f32 rows: added one contact after the other, in f32)."""
    flat = vals.reshape(len(vals), -1)
    if vals.dtype == np.float32:
        out = np.zeros((n, flat.shape[1]), np.float32)
        np.add.at(out, ci, flat)
        return out.reshape((n,) + vals.shape[1:])
    out = np.stack([np.bincount(ci, weights=flat[:, k], minlength=n) for k in range(flat.shape[1])], axis=1)
    return out.reshape((n,) + vals.shape[1:])


class ElasticityReading:
    def __init__(self, young_modulus, poisson_ratio, nonlinear_strain, kernel_density=CUBIC, kernel_gradient=CUBIC):
        self.d0, self.d1, self.d2 = coefficients(float(young_modulus), float(poisson_ratio))
        self.nonlinear = bool(nonlinear_strain)
        self.kd, self.kg = kernel_density, kernel_gradient
        self.positions0 = np.zeros((0, 3))
        self.volumes0 = np.zeros(0)
        self.rotations = np.zeros((0, 3, 3))
        self.off = np.zeros(1, np.int64)
        self.j = np.zeros(0, np.int64)

    # init (:84-112): quirk 1 (volumes0 / rotations are resized, not cleared) and quirk 2 (both endpoints of each directed contact)
    def init(self, h, positions, masses):
        n = len(positions)
        if len(self.positions0) == n:
            return False
        self.positions0 = np.asarray(positions, np.float64).copy()
        old = len(self.volumes0)
        v = np.zeros(n)
        v[:min(old, n)] = self.volumes0[:min(old, n)]
        R = np.tile(np.eye(3), (n, 1, 1))
        R[:min(old, n)] = self.rotations[:min(old, n)]
        self.rotations = R
        self.off, self.j = rest_contacts(np.asarray(positions, np.float32), h)
        ci = rows(self.off)
        w = kernel_w(np.linalg.norm(self.positions0[ci] - self.positions0[self.j], axis=1), h, self.kd)
        m = np.asarray(masses, np.float64)
        v += np.bincount(ci, weights=m[self.j] * w, minlength=n)
        v += np.bincount(self.j, weights=m[ci] * w, minlength=n)
        self.volumes0 = m / v
        return True

    def set_lists(self, h):
        self.off, self.j = rest_contacts(np.asarray(self.positions0, np.float32), h)

    # compute_rotations + compute_stresses (:115-262)
    def rotations_and_stresses(self, h, positions, masses, dtype=np.float64):
        n = len(positions)
        p = np.asarray(positions, dtype)
        m = np.asarray(masses, dtype)
        ci, cj = rows(self.off), self.j
        p0 = np.asarray(self.positions0, dtype)
        v0 = np.asarray(self.volumes0, dtype)
        pji = p[cj] - p[ci]
        p0ji = p0[cj] - p0[ci]
        d0 = p0[ci] - p0[cj]
        w = kernel_w(norm(d0, dtype), h, self.kd, dtype) * m[cj]
        A = segsum(ci, np.einsum("ni,nj->nij", pji, p0ji * w[:, None]), n)
        self.A_pq = A
        self.rotations = rotation_from_matrix_eps(A, self.rotations, dtype=dtype)
        g = gradient(d0, h, self.kg, dtype)
        self._g = g
        u = np.einsum("nji,nj->ni", self.rotations[ci], pji) - p0ji
        F = segsum(ci, np.einsum("ni,nj->nij", g * v0[cj][:, None], u), n)
        k = 0.564  # quirk 3
        C = np.array([[self.d0, self.d1, self.d1], [self.d1, self.d0, self.d1], [self.d1, self.d1, self.d0]], dtype)
        if self.nonlinear:
            J = F + np.eye(3, dtype=dtype)
            S = np.einsum("nij,nkj->nik", J, J)
            diag = np.einsum("ij,nj->ni", C, np.stack([S[:, 0, 0] - 1, S[:, 1, 1] - 1, S[:, 2, 2] - 1], axis=1)) * k
            off = np.stack([S[:, 1, 0], S[:, 2, 0], S[:, 2, 1]], axis=1) * k * self.d2
        else:
            diag = np.einsum("ij,nj->ni", C, np.stack([F[:, 0, 0], F[:, 1, 1], F[:, 2, 2]], axis=1))
            off = np.stack([F[:, 1, 0] + F[:, 0, 1], F[:, 2, 0] + F[:, 0, 2], F[:, 1, 2] + F[:, 2, 1]], axis=1) * k * self.d2
        self.grad_tr = F
        self.stress = np.concatenate([diag, off], axis=1)

    # the force loop of solve (:268-334), on the rotations, stresses and gradients the object holds
    def accelerations(self, volumes, density0, dtype=np.float64):
        n = len(self.volumes0)
        ci, cj = rows(self.off), self.j
        g, v0, s, F, R = (np.asarray(x, dtype) for x in (self._g, self.volumes0, self.stress, self.grad_tr, self.rotations))
        sd = sym_mul(s[ci], g * v0[cj][:, None])
        if self.nonlinear:
            sd = sd + np.einsum("nij,nj->ni", F[ci], sd)
        f_ji = sd * -v0[ci][:, None]
        sd = sym_mul(s[cj], g * -v0[ci][:, None])
        if self.nonlinear:
            sd = sd + np.einsum("nij,nj->ni", F[cj], sd)
        f_ij = sd * -v0[cj][:, None]
        force = (np.einsum("nij,nj->ni", R[cj], f_ij) - np.einsum("nij,nj->ni", R[ci], f_ji)) * 0.5
        return segsum(ci, force, n) / (np.asarray(volumes, dtype) * float(density0))[:, None]

    def step(self, h, positions, volumes, density0):
        """One `solve`: returns the accelerations it adds."""
        masses = np.asarray(volumes, np.float64) * density0
        self.init(h, positions, masses)
        self.rotations_and_stresses(h, positions, masses)
        return self.accelerations(volumes, density0)

    # NonPressureForce::solve, as a host force of salva_amd.LiquidWorld or of the CPU checker
    def solve(self, timestep, kernel_radius, fluid_fluid_contacts, fluid_boundaries_contacts, fluid, boundaries, densities):
        a = self.step(kernel_radius, np.asarray(fluid.positions), np.asarray(fluid.volumes, np.float64), float(fluid.density0))
        fluid.accelerations += a.astype(fluid.accelerations.dtype)
